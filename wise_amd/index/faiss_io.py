"""Reader/writer for the one faiss file layout WISE produces for flat search:
`faiss.write_index(IndexIDMap(IndexFlatIP(d)))` (reference: src/index/feature_search_index.py:47-52,84,96).

Layout restated from faiss's published index_write.cpp / index_read.cpp (faiss 1.7.x, little endian):

    u32  'IxMp'                                   IndexIDMap fourcc
    header: i32 d | i64 ntotal | i64 dummy(1<<20) | i64 dummy(1<<20) | u8 is_trained | i32 metric_type(0 = IP)
    u32  'IxFI'                                   IndexFlatIP fourcc
    header (same fields)
    u64  n_floats (= ntotal*d) | f32[n_floats]    the rows (1.7.2 writes xb as a float vector; newer versions
                                                  write the same bytes as a uint8 `codes` vector sized in 4-byte units)
    u64  ntotal | i64[ntotal]                     id_map

The IVF file the reference writes for index_type 'IndexIVFFlat' (feature_search_index.py:53-76,84) is restated the
same way (write_ivf_flat_ip / read_ivf_flat_ip below):

    u32  'IwFl'                                   IndexIVFFlat fourcc
    header (d, ntotal, ...) | u64 nlist | u64 nprobe
    u32  'IxFI' + header(d, nlist) + u64 n_floats + f32[nlist*d]      the coarse quantizer (centroids)
    u8   direct-map type (0 = none) | u64 0                           empty direct map
    u32  'ilar' | u64 nlist | u64 code_size (= 4*d)
    u32  'full' | u64 nlist | u64 sizes[nlist]        (or 'sprs' | u64 2*m | (list, size) pairs when most lists are empty)
    per non-empty list: u8 codes[size*code_size] (the fp32 rows) | i64 ids[size]

The file of index types 'IndexIVFPQ<m>' (write_ivf_pq_ip / read_ivf_pq_ip) restates faiss's IndexIVFPQ record:

    u32  'IwPQ'                                   IndexIVFPQ fourcc
    header | u64 nlist | u64 nprobe | 'IxFI' quantizer | direct map           exactly as in the 'IwFl' file
    u8   by_residual (1) | u64 code_size (= m)
    u64  d | u64 M | u64 nbits (8) | u64 n_floats (= 256*d) | f32[M*256*dsub] the ProductQuantizer record (centroids)
    'ilar' array inverted lists with code_size = m: per non-empty list u8 codes[size*m] | i64 ids[size]

The file of index types 'IndexIVFPQ<m>R8' / 'IndexIVFPQ<m>R16' (write_ivf_pq_refine_ip / read_ivf_pq_refine_ip) is THIS
REPOSITORY'S OWN FORMAT, not a faiss layout (faiss's 8-bit refine stores keep a range per dimension, these rows a scale per row):

    u32  'WiPR' | u32 version (1) | u32 kind (8 or 16) | u32 k_factor
    the complete 'IwPQ' record above
    u64  n_bytes | the compact rows in list order: i8[N*d] (kind 8) or bf16[N*d] (kind 16)
    u64  N | f32[N]                                                           the row scales (kind 8 only)

The file of index types 'IndexIVFOPQ<m>' and 'IndexIVFOPQ<m>R8' / 'R16' (write_ivf_opq_ip / read_ivf_opq_ip) is a wrapper of the same
kind, again THIS REPOSITORY'S OWN FORMAT (faiss writes an OPQMatrix inside an IndexPreTransform, which rotates the whole vector; this
rotation acts on the residual, after the coarse stage):

    u32  'WiOP' | u32 version (1) | u32 d
    f32[d*d]                                      the rotation R, row-major: a residual r is encoded as R r
    a complete 'IwPQ' record (IndexIVFOPQ<m>) or a complete 'WiPR' record (IndexIVFOPQ<m>R8 / R16)

The file of index type 'IndexIVFSQ8' (write_ivf_sq_ip / read_ivf_sq_ip) restates faiss's IndexIVFScalarQuantizer record:

    u32  'IwSq'                                   IndexIVFScalarQuantizer fourcc
    header | u64 nlist | u64 nprobe | 'IxFI' quantizer | direct map           exactly as in the 'IwFl' file
    i32  qtype (0 = QT_8bit, the first value of faiss's QuantizerType; 1 is QT_4bit) | i32 rangestat (0 = RS_minmax)
         | f32 rangestat_arg (0) | u64 d | u64 code_size (= d)
    u64  2d | f32[2d] trained                     vmin [d], then vdiff [d]
    u64  code_size (= d) | u8 by_residual (1)
    'ilar' array inverted lists with code_size = d: per non-empty list u8 codes[size*d] | i64 ids[size]

Under a process group with WISE_SHARDED_IVF=1 a rank's part file (`...faiss.part-RRR-of-WWW`) is a complete 'IwFl' / 'IwPQ' / 'WiPR' / 'WiOP' / 'IwSq' file
of the rank's rows with the list sizes clipped to them; the *_range readers cut the same slice out of a single file, opening only
the lists that overlap it.

faiss is not in the container, so these layouts are UNPINNED against a real faiss binary; the round
trip is pinned by tests/test_feature_store_index_io.py.  The rows are memory-mapped on read so a
158 GiB index (docs/Search-Index-Evaluation.md:109) streams to the GPU without a host copy.
"""
from __future__ import annotations

import struct
from pathlib import Path

import numpy as np

_DUMMY = 1 << 20
QT_8BIT = 0          # faiss ScalarQuantizer::QuantizerType::QT_8bit


def _fourcc(s: str) -> int:
    b = s.encode("ascii")
    return b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24)


def _header(d: int, ntotal: int, metric: int = 0) -> bytes:
    return struct.pack("<iqqq?i", d, ntotal, _DUMMY, _DUMMY, True, metric)


_HDR_SIZE = struct.calcsize("<iqqq?i")  # 4 + 8*3 + 1 + 4 = 33


def write_idmap_flat_ip(path, X: np.ndarray, ids: np.ndarray) -> None:
    X = np.ascontiguousarray(X, dtype=np.float32)
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    n, d = X.shape
    assert ids.shape == (n,)
    with open(path, "wb") as f:
        f.write(struct.pack("<I", _fourcc("IxMp")))
        f.write(_header(d, n))
        f.write(struct.pack("<I", _fourcc("IxFI")))
        f.write(_header(d, n))
        f.write(struct.pack("<Q", n * d))
        X.tofile(f)
        f.write(struct.pack("<Q", n))
        ids.tofile(f)


def _read_header(buf, off):
    d, ntotal, _, _, trained, metric = struct.unpack_from("<iqqq?i", buf, off)
    off += _HDR_SIZE
    if metric > 1:
        off += 4  # metric_arg
    return d, ntotal, metric, off


def read_idmap_flat_ip(path, mmap: bool = True):
    """-> (X [n,d] float32 (memmap view), ids int64[n]).  Raises RuntimeError like faiss on a missing file."""
    p = Path(path)
    if not p.exists():
        raise RuntimeError(f"Error: 'f' failed: could not open {p} for reading: No such file or directory")
    with open(p, "rb") as f:
        head = f.read(4 + _HDR_SIZE + 4 + 4 + _HDR_SIZE + 4 + 8)
    (cc,) = struct.unpack_from("<I", head, 0)
    if cc == _fourcc("IxFI"):  # a bare IndexFlatIP: ids are the positions
        d, n, metric, off = _read_header(head, 4)
        (cnt,) = struct.unpack_from("<Q", head, off)
        off += 8
        X = np.memmap(p, dtype=np.float32, mode="r", offset=off, shape=(n, d)) if mmap else \
            np.fromfile(p, dtype=np.float32, count=n * d, offset=off).reshape(n, d)
        return X, np.arange(n, dtype=np.int64)
    if cc != _fourcc("IxMp"):
        raise RuntimeError(f"{p}: index type 0x{cc:08x} is not IndexIDMap/IndexFlatIP; only flat IP indexes are "
                           f"supported by the MI355X search path")
    d, n, metric, off = _read_header(head, 4)
    (cc2,) = struct.unpack_from("<I", head, off)
    if cc2 != _fourcc("IxFI"):
        raise RuntimeError(f"{p}: IndexIDMap wraps index type 0x{cc2:08x}, expected IndexFlatIP")
    d2, n2, metric2, off = _read_header(head, off + 4)
    (cnt,) = struct.unpack_from("<Q", head, off)
    off += 8
    if cnt != n2 * d2 or d2 != d:
        raise RuntimeError(f"{p}: inconsistent flat payload ({cnt} values for {n2} x {d2})")
    X = np.memmap(p, dtype=np.float32, mode="r", offset=off, shape=(n2, d2)) if mmap else \
        np.fromfile(p, dtype=np.float32, count=n2 * d2, offset=off).reshape(n2, d2)
    off += cnt * 4
    with open(p, "rb") as f:
        f.seek(off)
        (nid,) = struct.unpack("<Q", f.read(8))
        ids = np.fromfile(f, dtype=np.int64, count=nid)
    if nid != n2:
        raise RuntimeError(f"{p}: id_map has {nid} entries for {n2} rows")
    return X, ids


def write_ivf_flat_ip(path, centroids: np.ndarray, X: np.ndarray, ids: np.ndarray, list_off: np.ndarray,
                      nprobe: int = 1) -> None:
    """X / ids hold the lists back to back; list l is rows list_off[l] .. list_off[l+1]-1."""
    centroids = np.ascontiguousarray(centroids, dtype=np.float32)
    X = np.ascontiguousarray(X, dtype=np.float32)
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    list_off = np.ascontiguousarray(list_off, dtype=np.int64)
    nlist, d = centroids.shape
    n = X.shape[0]
    assert X.shape == (n, d) and ids.shape == (n,) and list_off.shape == (nlist + 1,) and list_off[-1] == n
    sizes = (list_off[1:] - list_off[:-1]).astype(np.uint64)
    with open(path, "wb") as f:
        f.write(struct.pack("<I", _fourcc("IwFl")))
        f.write(_header(d, n))
        f.write(struct.pack("<QQ", nlist, nprobe))
        f.write(struct.pack("<I", _fourcc("IxFI")))
        f.write(_header(d, nlist))
        f.write(struct.pack("<Q", nlist * d))
        centroids.tofile(f)
        f.write(struct.pack("<BQ", 0, 0))
        f.write(struct.pack("<IQQ", _fourcc("ilar"), nlist, 4 * d))
        nonzero = np.flatnonzero(sizes)
        if len(nonzero) > nlist // 2:
            f.write(struct.pack("<IQ", _fourcc("full"), nlist))
            sizes.tofile(f)
        else:
            f.write(struct.pack("<IQ", _fourcc("sprs"), 2 * len(nonzero)))
            np.stack([nonzero.astype(np.uint64), sizes[nonzero]], axis=1).tofile(f)
        for l in nonzero:
            a, b = int(list_off[l]), int(list_off[l + 1])
            X[a:b].tofile(f)
            ids[a:b].tofile(f)


def _read_ivf_head(f, p, pq: bool = False, sq: bool = False):
    """Everything of an 'IwFl' file up to the list payload: (centroids, list_off, nprobe, start of the payload).
    pq: an 'IwPQ' file instead; the ProductQuantizer record read on the way is appended as (m, codebooks).
    sq: an 'IwSq' file instead; the ScalarQuantizer record's trained values [2d] are appended."""
    base = f.tell()                                          # (an 'IwPQ' record may sit inside a 'WiPR' file)
    (cc,) = struct.unpack("<I", f.read(4))
    want, name = ("IwPQ", "IndexIVFPQ") if pq else ("IwSq", "IndexIVFScalarQuantizer") if sq else ("IwFl", "IndexIVFFlat")
    if cc != _fourcc(want):
        raise RuntimeError(f"{p}: index type 0x{cc:08x} is not {name}")
    hdr = f.read(_HDR_SIZE + 4)
    d, n, metric, off = _read_header(hdr, 0)
    f.seek(base + 4 + off)
    nlist, nprobe = struct.unpack("<QQ", f.read(16))
    (cq,) = struct.unpack("<I", f.read(4))
    if cq != _fourcc("IxFI"):
        raise RuntimeError(f"{p}: coarse quantizer type 0x{cq:08x}, expected IndexFlatIP")
    pos = f.tell()
    hdr = f.read(_HDR_SIZE + 4)
    dq, nq_, _, off = _read_header(hdr, 0)
    f.seek(pos + off)
    (cnt,) = struct.unpack("<Q", f.read(8))
    if dq != d or nq_ != nlist or cnt != nlist * d:
        raise RuntimeError(f"{p}: inconsistent quantizer ({cnt} values for {nq_} x {dq})")
    centroids = np.fromfile(f, dtype=np.float32, count=cnt).reshape(nlist, d)
    (dm_type,) = struct.unpack("<B", f.read(1))
    (dm_n,) = struct.unpack("<Q", f.read(8))
    f.seek(8 * dm_n, 1)
    if dm_type == 2:  # hashtable pairs
        (npairs,) = struct.unpack("<Q", f.read(8))
        f.seek(16 * npairs, 1)
    m = codebooks = None
    if pq:
        by_residual, code_size_pq = struct.unpack("<BQ", f.read(9))
        dp, m, nbits, cnt = struct.unpack("<QQQQ", f.read(32))
        if by_residual != 1 or nbits != 8 or dp != d or m < 1 or d % m or code_size_pq != m or cnt != 256 * d:
            raise RuntimeError(f"{p}: unsupported IndexIVFPQ (by_residual={by_residual}, d={dp}, M={m}, nbits={nbits}, "
                               f"code_size={code_size_pq}, {cnt} codebook values)")
        codebooks = np.fromfile(f, dtype=np.float32, count=cnt).reshape(m, 256, d // m)
    trained = None
    if sq:
        qtype, rangestat, rangestat_arg, dsq, code_size_sq, cnt = struct.unpack("<iifQQQ", f.read(36))
        if qtype != QT_8BIT or dsq != d or code_size_sq != d or cnt != 2 * d:
            raise RuntimeError(f"{p}: unsupported IndexIVFScalarQuantizer (qtype={qtype}, d={dsq}, code_size={code_size_sq}, "
                               f"{cnt} trained values): QT_8bit with one range per dimension is what is read")
        trained = np.fromfile(f, dtype=np.float32, count=cnt)
        code_size_ivf, by_residual = struct.unpack("<QB", f.read(9))
        if trained.size != cnt or code_size_ivf != d or by_residual != 1:
            raise RuntimeError(f"{p}: unsupported IndexIVFScalarQuantizer (code_size={code_size_ivf}, by_residual={by_residual})")
    il, nl2, code_size = struct.unpack("<IQQ", f.read(20))
    if il != _fourcc("ilar") or nl2 != nlist or code_size != (m if pq else d if sq else 4 * d):
        raise RuntimeError(f"{p}: unexpected inverted lists (type 0x{il:08x}, code size {code_size})")
    (lt, vn) = struct.unpack("<IQ", f.read(12))
    sizes = np.zeros(nlist, dtype=np.int64)
    if lt == _fourcc("full"):
        sizes[:] = np.fromfile(f, dtype=np.uint64, count=vn).astype(np.int64)
    elif lt == _fourcc("sprs"):
        pairs = np.fromfile(f, dtype=np.uint64, count=vn).reshape(-1, 2).astype(np.int64)
        sizes[pairs[:, 0]] = pairs[:, 1]
    else:
        raise RuntimeError(f"{p}: unknown list layout 0x{lt:08x}")
    list_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    if list_off[-1] != n:
        raise RuntimeError(f"{p}: lists hold {list_off[-1]} rows, header says {n}")
    if pq:
        return centroids, list_off, int(nprobe), f.tell(), int(m), codebooks
    if sq:
        return centroids, list_off, int(nprobe), f.tell(), trained
    return centroids, list_off, int(nprobe), f.tell()


def _missing(p):
    return RuntimeError(f"Error: 'f' failed: could not open {p} for reading: No such file or directory")


def read_ivf_flat_ip(path):
    """-> dict(centroids [nlist,d], X [n,d], ids [n], list_off [nlist+1], nprobe).  The lists are returned back to
    back in list order, which is the layout the search kernel wants."""
    p = Path(path)
    if not p.exists():
        raise _missing(p)
    with open(p, "rb") as f:
        centroids, list_off, nprobe, _ = _read_ivf_head(f, p)
        d, n = centroids.shape[1], int(list_off[-1])
        X = np.empty((n, d), dtype=np.float32)
        ids = np.empty((n,), dtype=np.int64)
        for l in np.flatnonzero(np.diff(list_off)):
            a, b = int(list_off[l]), int(list_off[l + 1])
            X[a:b] = np.fromfile(f, dtype=np.float32, count=(b - a) * d).reshape(b - a, d)
            ids[a:b] = np.fromfile(f, dtype=np.int64, count=b - a)
    return {"centroids": centroids, "X": X, "ids": ids, "list_off": list_off, "nprobe": nprobe}


def ivf_flat_ip_ntotal(path) -> int:
    """Rows of an 'IwFl' file (its header), without reading the lists."""
    p = Path(path)
    if not p.exists():
        raise _missing(p)
    with open(p, "rb") as f:
        (cc,) = struct.unpack("<I", f.read(4))
        if cc != _fourcc("IwFl"):
            raise RuntimeError(f"{p}: index type 0x{cc:08x} is not IndexIVFFlat")
        return int(_read_header(f.read(_HDR_SIZE + 4), 0)[1])


def read_ivf_flat_ip_range(path, lo: int, hi: int):
    """Rows [lo, hi) of the list-major array read_ivf_flat_ip returns, reading only the lists that overlap the range
    (one rank's slice of an index sharded across GPUs: wise_amd/index/sharded.py).
    -> dict(centroids [nlist,d] (all of them), X [hi-lo,d], ids [hi-lo], list_off [nlist+1] = clip(list_off - lo, 0,
    hi - lo), nprobe).  List l's payload sits at list_off[l] * (4d + 8) bytes into the payload (rows, then ids)."""
    p = Path(path)
    if not p.exists():
        raise _missing(p)
    with open(p, "rb") as f:
        centroids, list_off, nprobe, data = _read_ivf_head(f, p)
        d, n = centroids.shape[1], int(list_off[-1])
        lo, hi = int(lo), int(hi)
        if not (0 <= lo <= hi <= n):
            raise ValueError(f"read_ivf_flat_ip_range: [{lo}, {hi}) outside [0, {n}]")
        X = np.empty((hi - lo, d), dtype=np.float32)
        ids = np.empty((hi - lo,), dtype=np.int64)
        sizes = np.diff(list_off)
        first = int(np.searchsorted(list_off, lo, side="right")) - 1     # the list that holds row lo
        for l in range(max(first, 0), len(sizes)):
            s0, s1 = int(list_off[l]), int(list_off[l + 1])
            if s0 >= hi:
                break
            a, b = max(s0, lo), min(s1, hi)
            if a >= b:
                continue
            base = data + s0 * (4 * d + 8)
            f.seek(base + (a - s0) * 4 * d)
            X[a - lo:b - lo] = np.fromfile(f, dtype=np.float32, count=(b - a) * d).reshape(b - a, d)
            f.seek(base + (s1 - s0) * 4 * d + (a - s0) * 8)
            ids[a - lo:b - lo] = np.fromfile(f, dtype=np.int64, count=b - a)
    return {"centroids": centroids, "X": X, "ids": ids, "list_off": np.clip(list_off - lo, 0, hi - lo),
            "nprobe": nprobe}


def write_ivf_pq_ip(path, centroids: np.ndarray, codebooks: np.ndarray, codes: np.ndarray, ids: np.ndarray,
                    list_off: np.ndarray, nprobe: int = 1) -> None:
    """codes [n,m] uint8 / ids hold the lists back to back; codebooks [m,256,d/m] fp32 (8-bit codes, by_residual)."""
    centroids = np.ascontiguousarray(centroids, dtype=np.float32)
    codebooks = np.ascontiguousarray(codebooks, dtype=np.float32)
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    list_off = np.ascontiguousarray(list_off, dtype=np.int64)
    nlist, d = centroids.shape
    n, m = codes.shape
    assert d % m == 0 and codebooks.shape == (m, 256, d // m)
    assert ids.shape == (n,) and list_off.shape == (nlist + 1,) and list_off[-1] == n
    with open(path, "wb") as f:
        _write_ivf_pq_record(f, centroids, codebooks, codes, ids, list_off, nprobe)


def _write_ivf_pq_record(f, centroids, codebooks, codes, ids, list_off, nprobe) -> None:
    (nlist, d), (n, m) = centroids.shape, codes.shape
    sizes = (list_off[1:] - list_off[:-1]).astype(np.uint64)
    f.write(struct.pack("<I", _fourcc("IwPQ")))
    f.write(_header(d, n))
    f.write(struct.pack("<QQ", nlist, nprobe))
    f.write(struct.pack("<I", _fourcc("IxFI")))
    f.write(_header(d, nlist))
    f.write(struct.pack("<Q", nlist * d))
    centroids.tofile(f)
    f.write(struct.pack("<BQ", 0, 0))
    f.write(struct.pack("<BQ", 1, m))                        # by_residual, code_size
    f.write(struct.pack("<QQQQ", d, m, 8, 256 * d))          # ProductQuantizer: d, M, nbits, centroids
    codebooks.tofile(f)
    f.write(struct.pack("<IQQ", _fourcc("ilar"), nlist, m))
    nonzero = np.flatnonzero(sizes)
    if len(nonzero) > nlist // 2:
        f.write(struct.pack("<IQ", _fourcc("full"), nlist))
        sizes.tofile(f)
    else:
        f.write(struct.pack("<IQ", _fourcc("sprs"), 2 * len(nonzero)))
        np.stack([nonzero.astype(np.uint64), sizes[nonzero]], axis=1).tofile(f)
    for l in nonzero:
        a, b = int(list_off[l]), int(list_off[l + 1])
        codes[a:b].tofile(f)
        ids[a:b].tofile(f)


def _read_ivf_pq_record(f, p):
    centroids, list_off, nprobe, _, m, codebooks = _read_ivf_head(f, p, pq=True)
    n = int(list_off[-1])
    codes = np.empty((n, m), dtype=np.uint8)
    ids = np.empty((n,), dtype=np.int64)
    for l in np.flatnonzero(np.diff(list_off)):
        a, b = int(list_off[l]), int(list_off[l + 1])
        codes[a:b] = np.fromfile(f, dtype=np.uint8, count=(b - a) * m).reshape(b - a, m)
        ids[a:b] = np.fromfile(f, dtype=np.int64, count=b - a)
    return {"centroids": centroids, "codebooks": codebooks, "codes": codes, "ids": ids, "list_off": list_off,
            "nprobe": nprobe}


def _read_ivf_pq_record_range(f, p, lo: int, hi: int):
    """Rows [lo, hi) of the list-major arrays of an 'IwPQ' record, reading only the lists that overlap the range.  List l's
    payload sits at list_off[l] * (m + 8) bytes into the payload (codes, then ids).  -> (dict with list_off clipped, n, end of the
    record)."""
    centroids, list_off, nprobe, data, m, codebooks = _read_ivf_head(f, p, pq=True)
    n = int(list_off[-1])
    lo, hi = int(lo), int(hi)
    if not (0 <= lo <= hi <= n):
        raise ValueError(f"read_ivf_pq_ip_range: [{lo}, {hi}) outside [0, {n}]")
    codes = np.empty((hi - lo, m), dtype=np.uint8)
    ids = np.empty((hi - lo,), dtype=np.int64)
    first = int(np.searchsorted(list_off, lo, side="right")) - 1         # the list that holds row lo
    for l in range(max(first, 0), len(list_off) - 1):
        s0, s1 = int(list_off[l]), int(list_off[l + 1])
        if s0 >= hi:
            break
        a, b = max(s0, lo), min(s1, hi)
        if a >= b:
            continue
        base = data + s0 * (m + 8)
        f.seek(base + (a - s0) * m)
        codes[a - lo:b - lo] = np.fromfile(f, dtype=np.uint8, count=(b - a) * m).reshape(b - a, m)
        f.seek(base + (s1 - s0) * m + (a - s0) * 8)
        ids[a - lo:b - lo] = np.fromfile(f, dtype=np.int64, count=b - a)
    out = {"centroids": centroids, "codebooks": codebooks, "codes": codes, "ids": ids, "list_off": np.clip(list_off - lo, 0, hi - lo),
           "nprobe": nprobe}
    return out, n, data + n * (m + 8)


def _pq_ntotal(f, p) -> int:
    (cc,) = struct.unpack("<I", f.read(4))
    if cc != _fourcc("IwPQ"):
        raise RuntimeError(f"{p}: index type 0x{cc:08x} is not IndexIVFPQ")
    return int(_read_header(f.read(_HDR_SIZE + 4), 0)[1])


def ivf_pq_ip_ntotal(path) -> int:
    """Rows of an 'IwPQ' file (its header), without reading the lists."""
    p = Path(path)
    if not p.exists():
        raise _missing(p)
    with open(p, "rb") as f:
        return _pq_ntotal(f, p)


def read_ivf_pq_ip_range(path, lo: int, hi: int):
    """Rows [lo, hi) of the list-major arrays read_ivf_pq_ip returns, reading only the lists that overlap the range (one rank's
    slice of an index sharded across GPUs: wise_amd/index/sharded.py).  -> the dict of read_ivf_pq_ip with codes [hi-lo,m],
    ids [hi-lo] and list_off = clip(list_off - lo, 0, hi - lo); centroids and codebooks are whole."""
    p = Path(path)
    if not p.exists():
        raise _missing(p)
    with open(p, "rb") as f:
        return _read_ivf_pq_record_range(f, p, lo, hi)[0]


def _read_refine_head(f, p):
    cc, version, kind, k_factor = struct.unpack("<IIII", f.read(16))
    if cc != _fourcc("WiPR") or version != 1 or kind not in (8, 16) or k_factor < 1:
        raise RuntimeError(f"{p}: not a re-ranking IndexIVFPQ file (type 0x{cc:08x}, version {version}, kind {kind}, "
                           f"k_factor {k_factor})")
    return int(kind), int(k_factor)


def ivf_pq_refine_ip_ntotal(path) -> int:
    """Rows of a 'WiPR' file (the header of its 'IwPQ' record), without reading the lists."""
    p = Path(path)
    if not p.exists():
        raise _missing(p)
    with open(p, "rb") as f:
        _read_refine_head(f, p)
        return _pq_ntotal(f, p)


def read_ivf_pq_refine_ip_range(path, lo: int, hi: int):
    """read_ivf_pq_ip_range for a 'WiPR' file: also rows [lo, hi) of the compact rows and of the scales, read by position (they
    are stored in list order as two plain arrays).  -> the dict of read_ivf_pq_refine_ip over the slice."""
    p = Path(path)
    if not p.exists():
        raise _missing(p)
    with open(p, "rb") as f:
        return _read_refine_record_range(f, p, lo, hi)


def _read_refine_record_range(f, p, lo: int, hi: int):
    """read_ivf_pq_refine_ip_range on an open file that stands at a 'WiPR' record"""
    kind, k_factor = _read_refine_head(f, p)
    out, n, end = _read_ivf_pq_record_range(f, p, lo, hi)
    lo, hi, d = int(lo), int(hi), out["centroids"].shape[1]
    width = d * (1 if kind == 8 else 2)
    f.seek(end)
    (nbytes,) = struct.unpack("<Q", f.read(8))
    if nbytes != n * width:
        raise RuntimeError(f"{p}: {nbytes} bytes of compact rows for {n} x {d} of kind {kind}")
    f.seek(end + 8 + lo * width)
    rows = np.fromfile(f, dtype=np.int8 if kind == 8 else np.uint16, count=(hi - lo) * d).reshape(hi - lo, d)
    scales = None
    if kind == 8:
        f.seek(end + 8 + n * width)
        (ns,) = struct.unpack("<Q", f.read(8))
        if ns != n:
            raise RuntimeError(f"{p}: {ns} scales for {n} rows")
        f.seek(end + 8 + n * width + 8 + lo * 4)
        scales = np.fromfile(f, dtype=np.float32, count=hi - lo)
    out.update(kind=kind, k_factor=k_factor, rows=rows, scales=scales)
    return out


def read_ivf_pq_ip(path):
    """-> dict(centroids [nlist,d], codebooks [m,256,d/m], codes [n,m] uint8, ids [n], list_off [nlist+1], nprobe), the
    lists back to back in list order."""
    p = Path(path)
    if not p.exists():
        raise _missing(p)
    with open(p, "rb") as f:
        return _read_ivf_pq_record(f, p)


def write_ivf_pq_refine_ip(path, centroids, codebooks, codes, ids, list_off, kind: int, k_factor: int, rows: np.ndarray,
                           scales=None, nprobe: int = 1) -> None:
    """An 'IwPQ' record plus the compact rows of a re-ranking index in the same list order: rows [n,d] int8 with scales [n]
    fp32 (kind 8) or rows [n,d] uint16 bf16 bit patterns (kind 16).  This repository's own format (module docstring)."""
    centroids = np.ascontiguousarray(centroids, dtype=np.float32)
    codebooks = np.ascontiguousarray(codebooks, dtype=np.float32)
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    list_off = np.ascontiguousarray(list_off, dtype=np.int64)
    nlist, d = centroids.shape
    n, m = codes.shape
    assert kind in (8, 16) and k_factor >= 1
    rows = np.ascontiguousarray(rows, dtype=np.int8 if kind == 8 else np.uint16)
    assert d % m == 0 and codebooks.shape == (m, 256, d // m) and rows.shape == (n, d)
    assert ids.shape == (n,) and list_off.shape == (nlist + 1,) and list_off[-1] == n
    if kind == 8:
        scales = np.ascontiguousarray(scales, dtype=np.float32)
        assert scales.shape == (n,)
    with open(path, "wb") as f:
        _write_refine_record(f, centroids, codebooks, codes, ids, list_off, kind, k_factor, rows, scales, nprobe)


def _write_refine_record(f, centroids, codebooks, codes, ids, list_off, kind, k_factor, rows, scales, nprobe) -> None:
    f.write(struct.pack("<IIII", _fourcc("WiPR"), 1, kind, k_factor))
    _write_ivf_pq_record(f, centroids, codebooks, codes, ids, list_off, nprobe)
    f.write(struct.pack("<Q", rows.nbytes))
    rows.tofile(f)
    if kind == 8:
        f.write(struct.pack("<Q", rows.shape[0]))
        scales.tofile(f)


def read_ivf_pq_refine_ip(path):
    """-> the dict of read_ivf_pq_ip plus kind, k_factor, rows [n,d] (int8 / uint16 bf16 bits) and scales [n] (None for kind 16)."""
    p = Path(path)
    if not p.exists():
        raise _missing(p)
    with open(p, "rb") as f:
        return _read_refine_record(f, p)


def _read_refine_record(f, p):
    """read_ivf_pq_refine_ip on an open file that stands at a 'WiPR' record"""
    kind, k_factor = _read_refine_head(f, p)
    out = _read_ivf_pq_record(f, p)
    n, d = out["codes"].shape[0], out["centroids"].shape[1]
    (nbytes,) = struct.unpack("<Q", f.read(8))
    if nbytes != n * d * (1 if kind == 8 else 2):
        raise RuntimeError(f"{p}: {nbytes} bytes of compact rows for {n} x {d} of kind {kind}")
    rows = np.fromfile(f, dtype=np.int8 if kind == 8 else np.uint16, count=n * d).reshape(n, d)
    scales = None
    if kind == 8:
        (ns,) = struct.unpack("<Q", f.read(8))
        if ns != n:
            raise RuntimeError(f"{p}: {ns} scales for {n} rows")
        scales = np.fromfile(f, dtype=np.float32, count=n)
    out.update(kind=int(kind), k_factor=int(k_factor), rows=rows, scales=scales)
    return out


# ---------------------------------------------------------------------------------------------- 'WiOP': a rotation + a PQ record
def write_ivf_opq_ip(path, rotation: np.ndarray, centroids, codebooks, codes, ids, list_off, nprobe: int = 1, kind=None,
                     k_factor=None, rows=None, scales=None) -> None:
    """The file of IndexIVFOPQ<m> (kind None: wraps an 'IwPQ' record) and IndexIVFOPQ<m>R8 / R16 (kind 8 / 16 with k_factor, rows
    and scales as write_ivf_pq_refine_ip takes them: wraps a 'WiPR' record).  rotation [d,d] fp32, row-major.  This repository's own
    format (module docstring)."""
    centroids = np.ascontiguousarray(centroids, dtype=np.float32)
    codebooks = np.ascontiguousarray(codebooks, dtype=np.float32)
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    list_off = np.ascontiguousarray(list_off, dtype=np.int64)
    rotation = np.ascontiguousarray(rotation, dtype=np.float32)
    nlist, d = centroids.shape
    n, m = codes.shape
    assert rotation.shape == (d, d) and d % m == 0 and codebooks.shape == (m, 256, d // m)
    assert ids.shape == (n,) and list_off.shape == (nlist + 1,) and list_off[-1] == n
    if kind is not None:
        assert kind in (8, 16) and k_factor is not None and k_factor >= 1
        rows = np.ascontiguousarray(rows, dtype=np.int8 if kind == 8 else np.uint16)
        assert rows.shape == (n, d)
        if kind == 8:
            scales = np.ascontiguousarray(scales, dtype=np.float32)
            assert scales.shape == (n,)
    with open(path, "wb") as f:
        f.write(struct.pack("<III", _fourcc("WiOP"), 1, d))
        rotation.tofile(f)
        if kind is None:
            _write_ivf_pq_record(f, centroids, codebooks, codes, ids, list_off, nprobe)
        else:
            _write_refine_record(f, centroids, codebooks, codes, ids, list_off, kind, k_factor, rows, scales, nprobe)


def _read_opq_head(f, p):
    """-> (rotation [d,d], fourcc of the wrapped record); the file then stands at that record"""
    cc, version, d = struct.unpack("<III", f.read(12))
    if cc != _fourcc("WiOP") or version != 1 or d < 1 or d > 1 << 16:
        raise RuntimeError(f"{p}: not an IndexIVFOPQ file (type 0x{cc:08x}, version {version}, d {d})")
    rotation = np.fromfile(f, dtype=np.float32, count=d * d)
    if rotation.size != d * d:
        raise RuntimeError(f"{p}: the rotation of an IndexIVFOPQ file is cut short ({rotation.size} of {d} x {d} values)")
    here = f.tell()
    (inner,) = struct.unpack("<I", f.read(4))
    f.seek(here)
    if inner not in (_fourcc("IwPQ"), _fourcc("WiPR")):
        raise RuntimeError(f"{p}: an IndexIVFOPQ file wraps record type 0x{inner:08x}, expected 'IwPQ' or 'WiPR'")
    return rotation.reshape(d, d), inner


def _with_rotation(out, rotation, p):
    if out["centroids"].shape[1] != rotation.shape[0]:
        raise RuntimeError(f"{p}: a rotation of d = {rotation.shape[0]} in front of an index of d = {out['centroids'].shape[1]}")
    out["rotation"] = rotation
    return out


def read_ivf_opq_ip(path):
    """-> the dict of read_ivf_pq_ip or of read_ivf_pq_refine_ip (the latter has 'kind'), plus rotation [d,d] fp32."""
    p = Path(path)
    if not p.exists():
        raise _missing(p)
    with open(p, "rb") as f:
        rotation, inner = _read_opq_head(f, p)
        return _with_rotation(_read_ivf_pq_record(f, p) if inner == _fourcc("IwPQ") else _read_refine_record(f, p), rotation, p)


def ivf_opq_ip_ntotal(path) -> int:
    """Rows of a 'WiOP' file (the header of its 'IwPQ' record), without reading the lists."""
    p = Path(path)
    if not p.exists():
        raise _missing(p)
    with open(p, "rb") as f:
        _, inner = _read_opq_head(f, p)
        if inner == _fourcc("WiPR"):
            _read_refine_head(f, p)
        return _pq_ntotal(f, p)


def read_ivf_opq_ip_range(path, lo: int, hi: int):
    """Rows [lo, hi) of the list-major arrays read_ivf_opq_ip returns, as read_ivf_pq_ip_range / read_ivf_pq_refine_ip_range cut them
    out of the wrapped record; the rotation is whole."""
    p = Path(path)
    if not p.exists():
        raise _missing(p)
    with open(p, "rb") as f:
        rotation, inner = _read_opq_head(f, p)
        out = _read_ivf_pq_record_range(f, p, lo, hi)[0] if inner == _fourcc("IwPQ") else _read_refine_record_range(f, p, lo, hi)
        return _with_rotation(out, rotation, p)


# ---------------------------------------------------------------------------------------------- 'IwSq': 8-bit scalar quantizer
def write_ivf_sq_ip(path, centroids: np.ndarray, trained: np.ndarray, codes: np.ndarray, ids: np.ndarray, list_off: np.ndarray,
                    nprobe: int = 1) -> None:
    """codes [n,d] uint8 / ids hold the lists back to back; trained [2d] fp32 = vmin, then vdiff (QT_8bit, by_residual)."""
    centroids = np.ascontiguousarray(centroids, dtype=np.float32)
    trained = np.ascontiguousarray(trained, dtype=np.float32)
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    list_off = np.ascontiguousarray(list_off, dtype=np.int64)
    nlist, d = centroids.shape
    n = codes.shape[0]
    assert codes.shape == (n, d) and trained.shape == (2 * d,)
    assert ids.shape == (n,) and list_off.shape == (nlist + 1,) and list_off[-1] == n
    sizes = (list_off[1:] - list_off[:-1]).astype(np.uint64)
    with open(path, "wb") as f:
        f.write(struct.pack("<I", _fourcc("IwSq")))
        f.write(_header(d, n))
        f.write(struct.pack("<QQ", nlist, nprobe))
        f.write(struct.pack("<I", _fourcc("IxFI")))
        f.write(_header(d, nlist))
        f.write(struct.pack("<Q", nlist * d))
        centroids.tofile(f)
        f.write(struct.pack("<BQ", 0, 0))
        f.write(struct.pack("<iifQQ", QT_8BIT, 0, 0.0, d, d))          # ScalarQuantizer: qtype, rangestat, rangestat_arg, d, code_size
        f.write(struct.pack("<Q", 2 * d))
        trained.tofile(f)
        f.write(struct.pack("<QB", d, 1))                        # code_size, by_residual
        f.write(struct.pack("<IQQ", _fourcc("ilar"), nlist, d))
        nonzero = np.flatnonzero(sizes)
        if len(nonzero) > nlist // 2:
            f.write(struct.pack("<IQ", _fourcc("full"), nlist))
            sizes.tofile(f)
        else:
            f.write(struct.pack("<IQ", _fourcc("sprs"), 2 * len(nonzero)))
            np.stack([nonzero.astype(np.uint64), sizes[nonzero]], axis=1).tofile(f)
        for l in nonzero:
            a, b = int(list_off[l]), int(list_off[l + 1])
            codes[a:b].tofile(f)
            ids[a:b].tofile(f)


def read_ivf_sq_ip(path):
    """-> dict(centroids [nlist,d], trained [2d] (vmin, then vdiff), codes [n,d] uint8, ids [n], list_off [nlist+1], nprobe), the
    lists back to back in list order.  A file cut short is refused (RuntimeError)."""
    p = Path(path)
    if not p.exists():
        raise _missing(p)
    with open(p, "rb") as f:
        try:
            centroids, list_off, nprobe, _, trained = _read_ivf_head(f, p, sq=True)
        except (struct.error, ValueError) as e:
            raise RuntimeError(f"{p}: the head of an IndexIVFScalarQuantizer file is cut short ({e})") from None
        n, d = int(list_off[-1]), centroids.shape[1]
        codes = np.empty((n, d), dtype=np.uint8)
        ids = np.empty((n,), dtype=np.int64)
        for l in np.flatnonzero(np.diff(list_off)):
            a, b = int(list_off[l]), int(list_off[l + 1])
            c = np.fromfile(f, dtype=np.uint8, count=(b - a) * d)
            i = np.fromfile(f, dtype=np.int64, count=b - a)
            if c.size != (b - a) * d or i.size != b - a:
                raise RuntimeError(f"{p}: list {l} is cut short ({c.size} code bytes and {i.size} ids for {b - a} rows)")
            codes[a:b], ids[a:b] = c.reshape(b - a, d), i
    return {"centroids": centroids, "trained": trained, "codes": codes, "ids": ids, "list_off": list_off, "nprobe": nprobe}


def ivf_sq_ip_ntotal(path) -> int:
    """Rows of an 'IwSq' file (its header), without reading the lists."""
    p = Path(path)
    if not p.exists():
        raise _missing(p)
    with open(p, "rb") as f:
        (cc,) = struct.unpack("<I", f.read(4))
        if cc != _fourcc("IwSq"):
            raise RuntimeError(f"{p}: index type 0x{cc:08x} is not IndexIVFScalarQuantizer")
        return int(_read_header(f.read(_HDR_SIZE + 4), 0)[1])


def read_ivf_sq_ip_range(path, lo: int, hi: int):
    """Rows [lo, hi) of the list-major arrays read_ivf_sq_ip returns, reading only the lists that overlap the range (one rank's
    slice of an index sharded across GPUs: wise_amd/index/sharded.py).  -> the dict of read_ivf_sq_ip with codes [hi-lo,d],
    ids [hi-lo] and list_off = clip(list_off - lo, 0, hi - lo); centroids and trained are whole.  List l's payload sits at
    list_off[l] * (d + 8) bytes into the payload (codes, then ids)."""
    p = Path(path)
    if not p.exists():
        raise _missing(p)
    with open(p, "rb") as f:
        try:
            centroids, list_off, nprobe, data, trained = _read_ivf_head(f, p, sq=True)
        except (struct.error, ValueError) as e:
            raise RuntimeError(f"{p}: the head of an IndexIVFScalarQuantizer file is cut short ({e})") from None
        n, d = int(list_off[-1]), centroids.shape[1]
        lo, hi = int(lo), int(hi)
        if not (0 <= lo <= hi <= n):
            raise ValueError(f"read_ivf_sq_ip_range: [{lo}, {hi}) outside [0, {n}]")
        codes = np.empty((hi - lo, d), dtype=np.uint8)
        ids = np.empty((hi - lo,), dtype=np.int64)
        first = int(np.searchsorted(list_off, lo, side="right")) - 1         # the list that holds row lo
        for l in range(max(first, 0), len(list_off) - 1):
            s0, s1 = int(list_off[l]), int(list_off[l + 1])
            if s0 >= hi:
                break
            a, b = max(s0, lo), min(s1, hi)
            if a >= b:
                continue
            base = data + s0 * (d + 8)
            f.seek(base + (a - s0) * d)
            c = np.fromfile(f, dtype=np.uint8, count=(b - a) * d)
            f.seek(base + (s1 - s0) * d + (a - s0) * 8)
            i = np.fromfile(f, dtype=np.int64, count=b - a)
            if c.size != (b - a) * d or i.size != b - a:
                raise RuntimeError(f"{p}: list {l} is cut short ({c.size} code bytes and {i.size} ids for {b - a} rows)")
            codes[a - lo:b - lo], ids[a - lo:b - lo] = c.reshape(b - a, d), i
    return {"centroids": centroids, "trained": trained, "codes": codes, "ids": ids, "list_off": np.clip(list_off - lo, 0, hi - lo),
            "nprobe": nprobe}


def index_fourcc(path) -> str:
    with open(path, "rb") as f:
        return f.read(4).decode("ascii", errors="replace")
