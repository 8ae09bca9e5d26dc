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

The file of index type 'IndexIVFSQfp16' (write_ivf_sq16_ip; read by the same readers) is the same faiss record with the other
quantizer type WISE builds — faiss's QT_fp16, which trains nothing:

    u32  'IwSq' ... direct map                                                 as above
    i32  qtype (4 = QT_fp16) | i32 rangestat (0) | f32 rangestat_arg (0) | u64 d | u64 code_size (= 2d)
    u64  0                                        the trained vector: empty
    u64  code_size (= 2d) | u8 by_residual (1)
    'ilar' array inverted lists with code_size = 2d: per non-empty list f16[size*d] (IEEE binary16, little endian) | i64 ids[size]

Its reader's dict has 'halves' [n,d] float16 where the QT_8bit dict has 'codes' and 'trained'.  Like the other records this one
is restated from the format and unpinned against a faiss-written file.

The file of index type 'IndexSQfp16' (write_idmap_sq16_ip / read_idmap_sq16_ip) is the flat file above with faiss's
IndexScalarQuantizer(d, QT_fp16, METRIC_INNER_PRODUCT) in the place of the IndexFlatIP:

    u32  'IxMp' | header                          IndexIDMap, as in the flat file
    u32  'IxSQ' | header                          IndexScalarQuantizer fourcc
    i32  qtype (4 = QT_fp16) | i32 rangestat (0) | f32 rangestat_arg (0) | u64 d | u64 code_size (= 2d)
    u64  0                                        the trained vector: empty          (the ScalarQuantizer record of 'IwSq', qtype 4)
    u64  n_bytes (= ntotal*2d) | f16[ntotal*d]    the codes vector: the rows as IEEE binary16, little endian
    u64  ntotal | i64[ntotal]                     id_map

A bare 'IxSQ' file (no id map) reads with ids equal to positions.  index_fourcc(path, inner=True) names the index an 'IxMp' file
wraps ('IxFI' or 'IxSQ'); read_index / read_index_range / index_ntotal serve this file too (dict(halves, ids)), and write_index
writes it for a state of 'halves' and 'ids' alone.  A rank's part of a row-sharded index is a complete file of its rows.

The file of index type 'IndexSQ8bit' (write_idmap_sq8_ip / read_idmap_sq8_ip, _range, idmap_sq8_ip_ntotal) is the same 'IxMp' around
'IxSQ' with faiss's QT_8bit record, RS_minmax with argument 0:

    u32  'IxMp' | header | u32 'IxSQ' | header    as above
    i32  qtype (0 = QT_8bit) | i32 rangestat (0) | f32 rangestat_arg (0) | u64 d | u64 code_size (= d)
    u64  2d | f32[2d]                             the trained vector: vmin [d], then vdiff [d]
    u64  n_bytes (= ntotal*d) | u8[ntotal*d]      the codes vector: one byte per dimension
    u64  ntotal | i64[ntotal]                     id_map

The record's qtype tells the two 'IxSQ' files apart (flat_sq_qtype); every field is validated per qtype, so a record that says qtype 0
with code_size 2d or without trained values is refused by file name, and neither reader takes the other's file.  read_index gives
dict(trained, codes, ids), and write_index writes the file for a state of 'trained', 'codes' and 'ids' without 'centroids'.

The file of index types 'IndexPQ<m>' (write_idmap_pq_ip / read_idmap_pq_ip, _range, idmap_pq_ip_ntotal) restates faiss's
IndexIDMap(IndexPQ(d, m, 8, METRIC_INNER_PRODUCT)) record — product-quantizer codes in row order, no lists:

    u32  'IxMp' | header | u32 'IxPq' | header(d, ntotal, ..., metric_type 0)
    u64  d | u64 M | u64 nbits (8) | u64 n_floats (= 256 d) | f32[M*256*dsub]     the ProductQuantizer record of 'IwPQ'
    u64  n_bytes (= ntotal*m) | u8[ntotal*m]                                     codes
    i32  search_type (0 = ST_PQ) | u8 encode_signs (0) | i32 polysemous_ht (8 m + 1, faiss's constructor default)
    u64  ntotal | i64[ntotal]                                                    id_map

The codes are memory-mapped on read; a bare 'IxPq' file (no id map) reads with ids equal to positions.  read_index gives
dict(codebooks, codes, ids), and write_index writes the file for a state of 'codebooks', 'codes' and 'ids' without 'centroids'.

The file of index types 'IndexPQ<m>R8' / 'IndexPQ<m>R16' (write_pq_refine_ip / read_pq_refine_ip, _range, pq_refine_ip_ntotal) is THIS
REPOSITORY'S OWN FORMAT, modelled on 'WiPR':

    u32  'WiFR' | u32 version (1) | u32 kind (8 or 16) | u32 k_factor
    the complete 'IxMp' record above
    u64  n_bytes | the compact rows in row order: i8[N*d] (kind 8) or bf16[N*d] (kind 16)
    u64  N | f32[N]                                                               the row scales (kind 8 only)

Every reader of either refuses a foreign, truncated or mismatched file by file name (n_bytes != ntotal*m, n_floats != 256 d,
nbits != 8, an id map of another length, ...).

The file of index type 'IndexFlatL2' (write_idmap_flat_l2 / read_idmap_flat_l2, _range, idmap_flat_l2_ntotal) is the flat file at the
top with faiss's IndexFlatL2 in the place of the IndexFlatIP: the inner fourcc is 'IxF2' and metric_type is 1 (METRIC_L2) in both
headers; everything else is the 'IxFI' layout, a bare 'IxF2' file reads with ids equal to positions, and _flat_head refuses by name
an 'IxFI' file whose metric_type is 1 and an 'IxF2' file whose metric_type is 0.

The IndexIVFFlatL2 file (write_ivf_flat_l2 / read_ivf_flat_l2 / read_ivf_flat_l2_range / ivf_flat_l2_ntotal) is faiss's
IndexIVFFlat(IndexFlatL2(d), d, nlist, METRIC_L2): the 'IwFl' record above with metric_type 1 in its header and an 'IxF2' quantizer
whose header says metric_type 1 too; everything else is the inner-product layout.  The record's metric_type tells the two 'IwFl'
files apart (read_index and its siblings dispatch on it), the L2 reader's dict carries metric='l2' (write_index picks the record by
that key), read_ivf_flat_ip refuses an L2 file at its quantizer's fourcc and the L2 readers refuse a metric-0 file by name.

Under a process group with WISE_SHARDED_IVF=1 a rank's part file (`...faiss.part-RRR-of-WWW`) is a complete 'IwFl' / 'IwPQ' / 'WiPR' / 'WiOP' / 'IwSq' file
of the rank's rows with the list sizes clipped to them; the *_range readers cut the same slice out of a single file, opening only
the lists that overlap it.

Every IVF record ends in the same inverted-list block, written and read by one piece of code (_write_lists, _read_lists,
_read_lists_range) that the payload's row width and dtype parameterise.  read_index / read_index_range / index_ntotal pick the named
reader by the file's fourcc and write_index the named writer by the state's keys; callers that do not care which family they hold
(feature_search_index.py) use those four.  The two flat files share their head too — the optional id map's header, the inner
fourcc and header, the ScalarQuantizer record of 'IxSQ', the payload's length — and one parser (_flat_head) and one id reader
(_flat_ids) serve every reader of either.

faiss is not in the container, so these layouts are UNPINNED against a real faiss binary; the round
trip is pinned by tests/test_feature_store_index_io.py.  The rows are memory-mapped on read so a
158 GiB index (docs/Search-Index-Evaluation.md:109) streams to the GPU without a host copy.
"""
from __future__ import annotations

import struct
from pathlib import Path
from typing import NamedTuple

import numpy as np

_DUMMY = 1 << 20
QT_8BIT = 0          # faiss ScalarQuantizer::QuantizerType::QT_8bit
QT_FP16 = 4          # ... QT_4bit, QT_8bit_uniform, QT_4bit_uniform, QT_fp16


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


class _FlatHead(NamedTuple):
    """The head of a flat file, 'IxFI', 'IxF2' or 'IxSQ', bare or inside 'IxMp' (_flat_head)."""
    inner: str           # 'IxFI' / 'IxF2' (fp32 rows, inner product / L2) or 'IxSQ' (binary16 rows, QT_fp16)
    d: int
    n: int
    off: int             # byte offset of the payload
    dtype: object        # of a payload value
    idmap: bool          # an id map follows the payload (else ids are the positions)
    trained: object = None   # [2d] float32 of an 'IxSQ' record of QT_8bit (vmin, then vdiff); None for every other flat file


_FLAT_HEAD_BYTES = 4 + (_HDR_SIZE + 4) + 4 + (_HDR_SIZE + 4) + 36 + 8     # the most a flat head takes: both headers with a metric_arg
_FLAT_NAMES = {"IxFI": "IndexFlatIP", "IxSQ": "IndexSQfp16", "IxF2": "IndexFlatL2"}
_SQ16_NAMES = {0: "IndexSQfp16", 1: "IndexSQfp16L2"}     # the two QT_fp16 'IxSQ' files, by the metric_type of their headers
_FLAT_METRIC = {"IxFI": 0, "IxF2": 1}     # faiss METRIC_INNER_PRODUCT / METRIC_L2: what the headers of an fp32 flat file must say


def _flat_outer(head: bytes):
    """(the fourcc the file opens with, the fourcc of the index — the one an 'IxMp' id map wraps, else the same —, the offset behind
    it, d and n of the id map's header or None); struct.error where the bytes end before that."""
    (cc,) = struct.unpack_from("<I", head, 0)
    if cc != _fourcc("IxMp"):
        return cc, cc, 4, None, None
    d0, n0, _, off = _read_header(head, 4)
    (inner,) = struct.unpack_from("<I", head, off)
    return cc, inner, off + 4, d0, n0


def _flat_head(p, want: str, qtype_want: int = QT_FP16, sq_metric=None) -> _FlatHead:
    """The head of the flat file `p`, which has to hold the index `want` ('IxFI' / 'IxF2' / 'IxSQ'), bare or inside 'IxMp'.  sq_metric: the
    metric_type both headers of a QT_fp16 'IxSQ' file must carry (0: IndexSQfp16, 1: IndexSQfp16L2; None: not looked at).  RuntimeError naming
    the file for anything else, a metric_type that is not the fourcc's ('IxFI': 0, 'IxF2': 1, in either header), a ScalarQuantizer record other than the one asked for (qtype_want: QT_fp16 with code_size 2d and no trained value, or QT_8bit with code_size d and 2d trained values), a payload length that is not n x d
    values, or a file shorter than its header promises."""
    size = p.stat().st_size
    with open(p, "rb") as f:
        head = f.read(_FLAT_HEAD_BYTES)
    try:
        cc, inner, off, d0, n0 = _flat_outer(head)
        idmap = cc == _fourcc("IxMp")
        metric0 = struct.unpack_from("<i", head, 4 + _HDR_SIZE - 4)[0] if idmap else None
        if inner != _fourcc(want):
            if want == "IxSQ":
                raise RuntimeError(f"{p}: index type 0x{inner:08x} is not IndexScalarQuantizer (IndexSQfp16: 'IxSQ', bare or inside 'IxMp')")
            if want == "IxF2":
                raise RuntimeError(f"{p}: index type 0x{inner:08x} is not IndexFlatL2 ('IxF2', bare or inside 'IxMp')")
            if idmap:
                raise RuntimeError(f"{p}: IndexIDMap wraps index type 0x{inner:08x}, expected IndexFlatIP")
            raise RuntimeError(f"{p}: index type 0x{cc:08x} is not IndexIDMap/IndexFlatIP; only flat IP indexes are "
                               f"supported by the MI355X search path")
        d, n, metric, off = _read_header(head, off)
        if want == "IxSQ":
            qtype, rangestat, rangestat_arg, dsq, code_size, ntrained = struct.unpack_from("<iifQQQ", head, off)
            off += 36
            if qtype_want == QT_8BIT and qtype == QT_8BIT and 0 < ntrained == 2 * d <= 2 * 65536:
                # the trained values stand between the record and the payload's length: read on from the file
                with open(p, "rb") as f:
                    f.seek(off)
                    trained = np.fromfile(f, dtype="<f4", count=int(ntrained))
                    tail = f.read(8)
                if trained.size != ntrained or len(tail) != 8:
                    raise struct.error("the trained values end early")
                off += 4 * int(ntrained)
                head = head[:off].ljust(off, b"\0") + tail
        (count,) = struct.unpack_from("<Q", head, off)
        off += 8
    except struct.error as e:
        name = "IndexSQ8bit" if want == "IxSQ" and qtype_want == QT_8BIT else _FLAT_NAMES[want]
        raise RuntimeError(f"{p}: the head of an {name} file is cut short ({e})") from None
    if want in _FLAT_METRIC and (metric != _FLAT_METRIC[want] or (idmap and metric0 != _FLAT_METRIC[want])):
        raise RuntimeError(f"{p}: an {_FLAT_NAMES[want]} file ('{want}') with metric_type {metric}"
                           + (f" under an IndexIDMap of metric_type {metric0}" if idmap else "")
                           + f": {_FLAT_NAMES[want]} is metric_type {_FLAT_METRIC[want]}")
    if want == "IxSQ" and qtype_want == QT_8BIT:
        if qtype != QT_8BIT or d < 1 or dsq != d or code_size != d or ntrained != 2 * d or (idmap and (d0 != d or n0 != n)):
            raise RuntimeError(f"{p}: unsupported IndexScalarQuantizer (qtype={qtype}, d={dsq} under a header of d={d}, "
                               f"code_size={code_size}, {ntrained} trained values): an IndexSQ8bit file is qtype 0 (QT_8bit) with "
                               f"code_size d and 2 d trained values")
        if n < 0 or count != n * d:
            raise RuntimeError(f"{p}: {count} code bytes for {n} x {d} 8-bit codes")
        need = off + n * d + ((8 + 8 * n) if idmap else 0)
        if size < need:
            raise RuntimeError(f"{p}: the file is cut short ({size} bytes, {need} promised by its header)")
        return _FlatHead(want, int(d), int(n), int(off), np.dtype(np.uint8), idmap, trained.astype(np.float32))
    if want == "IxSQ" and sq_metric is not None and qtype == QT_FP16 and (metric != sq_metric or (idmap and metric0 != sq_metric)):
        name = _SQ16_NAMES[sq_metric]
        raise RuntimeError(f"{p}: an {name} file ('IxSQ', qtype 4) with metric_type {metric}"
                           + (f" under an IndexIDMap of metric_type {metric0}" if idmap else "")
                           + f": {name} is metric_type {sq_metric} ({_SQ16_NAMES[1 - sq_metric]} is metric_type {1 - sq_metric})")
    if want == "IxSQ":
        if qtype != QT_FP16 or d < 1 or dsq != d or code_size != 2 * d or ntrained != 0 or (idmap and (d0 != d or n0 != n)):
            raise RuntimeError(f"{p}: unsupported IndexScalarQuantizer (qtype={qtype}, d={dsq} under a header of d={d}, "
                               f"code_size={code_size}, {ntrained} trained values): qtype 4 (QT_fp16) with code_size 2 d and no trained "
                               f"value is what is read")
        if n < 0 or count != n * 2 * d:
            raise RuntimeError(f"{p}: {count} code bytes for {n} x {d} binary16 values")
        dtype = np.dtype("<f2")
    else:
        if n < 0 or d < 1 or count != n * d or (idmap and d0 != d):
            raise RuntimeError(f"{p}: inconsistent flat payload ({count} values for {n} x {d})")
        dtype = np.dtype(np.float32)
    need = off + n * d * dtype.itemsize + ((8 + 8 * n) if idmap else 0)
    if size < need:
        raise RuntimeError(f"{p}: the file is cut short ({size} bytes, {need} promised by its header)")
    return _FlatHead(want, int(d), int(n), int(off), dtype, idmap)


def _flat_rows(p, head: _FlatHead, mmap: bool):
    """[n,d] payload of a flat file: a memmap view unless mmap is False (or there is no row to map)"""
    if mmap and head.n:
        return np.memmap(p, dtype=head.dtype, mode="r", offset=head.off, shape=(head.n, head.d))
    return np.fromfile(p, dtype=head.dtype, count=head.n * head.d, offset=head.off).reshape(head.n, head.d)


def _flat_ids(p, head: _FlatHead, lo: int, hi: int):
    """ids [lo, hi) of a flat file: the id map behind the payload, or the positions where the file has none"""
    if not head.idmap:
        return np.arange(lo, hi, dtype=np.int64)
    with open(p, "rb") as f:
        f.seek(head.off + head.n * head.d * head.dtype.itemsize)
        (nid,) = struct.unpack("<Q", f.read(8))
        if nid != head.n:
            raise RuntimeError(f"{p}: id_map has {nid} entries for {head.n} rows")
        f.seek(8 * lo, 1)
        ids = np.fromfile(f, dtype=np.int64, count=hi - lo)
    if ids.size != hi - lo:
        raise RuntimeError(f"{p}: the id_map is cut short ({ids.size} of {hi - lo} ids)")
    return ids


def read_idmap_flat_ip(path, mmap: bool = True):
    """-> (X [n,d] float32 (a memmap view unless mmap is False), ids int64[n]); a bare 'IxFI' file (no id map) gives ids = positions.
    Raises RuntimeError like faiss on a missing file, and naming the file for a truncated or foreign one."""
    p = _existing(path)
    head = _flat_head(p, "IxFI")
    return _flat_rows(p, head, mmap), _flat_ids(p, head, 0, head.n)


_IVF_RECORDS = {"IwFl": "IndexIVFFlat", "IwPQ": "IndexIVFPQ", "IwSq": "IndexIVFScalarQuantizer"}


def write_idmap_flat_l2(path, X: np.ndarray, ids: np.ndarray) -> None:
    """'IxMp' around 'IxF2' with metric_type 1 (METRIC_L2) in both headers; otherwise the 'IxFI' layout."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    n, d = X.shape
    assert ids.shape == (n,)
    with open(path, "wb") as f:
        f.write(struct.pack("<I", _fourcc("IxMp")))
        f.write(_header(d, n, 1))
        f.write(struct.pack("<I", _fourcc("IxF2")))
        f.write(_header(d, n, 1))
        f.write(struct.pack("<Q", n * d))
        X.tofile(f)
        f.write(struct.pack("<Q", n))
        ids.tofile(f)


def read_idmap_flat_l2(path, mmap: bool = True):
    """-> (X [n,d] float32 (a memmap view unless mmap is False), ids int64[n]) of an IndexFlatL2 file; a bare 'IxF2' file (no id map)
    gives ids = positions.  RuntimeError naming the file for a truncated or foreign one, or one whose metric_type is not 1."""
    p = _existing(path)
    head = _flat_head(p, "IxF2")
    return _flat_rows(p, head, mmap), _flat_ids(p, head, 0, head.n)


def read_idmap_flat_l2_range(path, lo: int, hi: int):
    """-> (X [hi - lo, d] float32, ids int64[hi - lo]): the rows [lo, hi) of an IndexFlatL2 file, read without mapping the rest."""
    p = _existing(path)
    head = _flat_head(p, "IxF2")
    if not (0 <= lo <= hi <= head.n):
        raise ValueError(f"{p}: rows [{lo}, {hi}) outside the file's {head.n}")
    X = np.fromfile(p, dtype=head.dtype, count=(hi - lo) * head.d, offset=head.off + lo * head.d * 4).reshape(hi - lo, head.d)
    return X, _flat_ids(p, head, lo, hi)


def idmap_flat_l2_ntotal(path) -> int:
    """ntotal of an IndexFlatL2 file, from its head alone."""
    return _flat_head(_existing(path), "IxF2").n


def _existing(path) -> Path:
    """path as a Path; RuntimeError like faiss on a missing file"""
    p = Path(path)
    if not p.exists():
        raise RuntimeError(f"Error: 'f' failed: could not open {p} for reading: No such file or directory")
    return p


def _expect_record(f, p, want: str) -> None:
    """Read the fourcc the file stands at; RuntimeError unless it is the IVF record `want`."""
    (cc,) = struct.unpack("<I", f.read(4))
    if cc != _fourcc(want):
        raise RuntimeError(f"{p}: index type 0x{cc:08x} is not {_IVF_RECORDS[want]}")


def _record_ntotal(f, p, want: str) -> int:
    """Rows of the IVF record `want` the file stands at (its header), without reading the lists."""
    _expect_record(f, p, want)
    return int(_read_header(f.read(_HDR_SIZE + 4), 0)[1])


def _ivf_arrays(centroids, ids, list_off, n: int):
    """What every IVF writer takes, as the contiguous arrays it writes: centroids [nlist,d] fp32, ids [n] and list_off [nlist+1]
    int64 (list l is rows list_off[l] .. list_off[l+1]-1 of the payload)."""
    centroids = np.ascontiguousarray(centroids, dtype=np.float32)
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    list_off = np.ascontiguousarray(list_off, dtype=np.int64)
    assert ids.shape == (n,) and list_off.shape == (centroids.shape[0] + 1,) and list_off[-1] == n
    return centroids, ids, list_off


def _write_ivf_head(f, record: str, centroids, n: int, nprobe: int, metric: int = 0) -> None:
    """What the 'IwFl', 'IwPQ' and 'IwSq' records open with: fourcc, header, nlist, nprobe, the 'IxFI' quantizer, an empty direct map.
    metric 1 (METRIC_L2, IndexIVFFlatL2): both headers say so and the quantizer is an 'IxF2' (IndexFlatL2)."""
    nlist, d = centroids.shape
    f.write(struct.pack("<I", _fourcc(record)))
    f.write(_header(d, n, metric))
    f.write(struct.pack("<QQ", nlist, nprobe))
    f.write(struct.pack("<I", _fourcc("IxF2" if metric == 1 else "IxFI")))
    f.write(_header(d, nlist, metric))
    f.write(struct.pack("<Q", nlist * d))
    centroids.tofile(f)
    f.write(struct.pack("<BQ", 0, 0))


def _write_lists(f, payload, ids, list_off) -> None:
    """The inverted-list block of every IVF record: the 'ilar' header with the payload's bytes per row as code_size, the 'full'
    (or, when most lists are empty, 'sprs') size table, then per non-empty list its payload rows followed by its ids."""
    nlist = list_off.shape[0] - 1
    sizes = (list_off[1:] - list_off[:-1]).astype(np.uint64)
    f.write(struct.pack("<IQQ", _fourcc("ilar"), nlist, payload.shape[1] * payload.dtype.itemsize))
    nonzero = np.flatnonzero(sizes)
    if len(nonzero) > nlist // 2:
        f.write(struct.pack("<IQ", _fourcc("full"), nlist))
        sizes.tofile(f)
    else:
        f.write(struct.pack("<IQ", _fourcc("sprs"), 2 * len(nonzero)))
        np.stack([nonzero.astype(np.uint64), sizes[nonzero]], axis=1).tofile(f)
    for l in nonzero:
        a, b = int(list_off[l]), int(list_off[l + 1])
        payload[a:b].tofile(f)
        ids[a:b].tofile(f)


def _read_lists_range(f, p, list_off, data: int, cols: int, dtype, lo: int, hi: int, who: str, strict: bool = False):
    """Rows [lo, hi) of the list-major (payload [n,cols] dtype, ids [n]) of a list block whose first list starts at byte `data`,
    reading only the lists that overlap the range: list l sits list_off[l] * (row bytes + 8) bytes in, its rows before its ids.
    who: the reader's name, for the ValueError of a range outside [0, n].  strict: a list cut short is a RuntimeError that names
    it ('IwSq'; the other records leave it to numpy's ValueError)."""
    n, lo, hi = int(list_off[-1]), int(lo), int(hi)
    if not (0 <= lo <= hi <= n):
        raise ValueError(f"{who}: [{lo}, {hi}) outside [0, {n}]")
    width = cols * np.dtype(dtype).itemsize
    payload = np.empty((hi - lo, cols), dtype=dtype)
    ids = np.empty((hi - lo,), dtype=np.int64)
    first = int(np.searchsorted(list_off, lo, side="right")) - 1         # the list that holds row lo
    for l in range(max(first, 0), len(list_off) - 1):
        s0, s1 = int(list_off[l]), int(list_off[l + 1])
        if s0 >= hi:
            break
        a, b = max(s0, lo), min(s1, hi)
        if a >= b:
            continue
        base = data + s0 * (width + 8)
        f.seek(base + (a - s0) * width)
        c = np.fromfile(f, dtype=dtype, count=(b - a) * cols)
        f.seek(base + (s1 - s0) * width + (a - s0) * 8)
        i = np.fromfile(f, dtype=np.int64, count=b - a)
        if strict and (c.size != (b - a) * cols or i.size != b - a):
            raise RuntimeError(f"{p}: list {l} is cut short ({c.size} code bytes and {i.size} ids for {b - a} rows)")
        payload[a - lo:b - lo], ids[a - lo:b - lo] = c.reshape(b - a, cols), i
    return payload, ids, np.clip(list_off - lo, 0, hi - lo)


def _read_lists(f, p, list_off, data: int, cols: int, dtype, strict: bool = False):
    """The whole list block: (payload [n,cols], ids [n]), the lists back to back in list order; the file is left at the block's end."""
    n = int(list_off[-1])
    payload, ids, _ = _read_lists_range(f, p, list_off, data, cols, dtype, 0, n, "", strict)
    f.seek(data + n * (cols * np.dtype(dtype).itemsize + 8))
    return payload, ids


# ---------------------------------------------------------------------------------------------- 'IwFl': fp32 rows
def write_ivf_flat_ip(path, centroids: np.ndarray, X: np.ndarray, ids: np.ndarray, list_off: np.ndarray,
                      nprobe: int = 1) -> None:
    """X / ids hold the lists back to back; list l is rows list_off[l] .. list_off[l+1]-1."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    centroids, ids, list_off = _ivf_arrays(centroids, ids, list_off, X.shape[0])
    assert X.shape == (X.shape[0], centroids.shape[1])
    with open(path, "wb") as f:
        _write_ivf_head(f, "IwFl", centroids, X.shape[0], nprobe)
        _write_lists(f, X, ids, list_off)


def _read_ivf_head(f, p, pq: bool = False, sq: bool = False, l2: bool = False):
    """Everything of an 'IwFl' file up to the list payload: (centroids, list_off, nprobe, start of the payload).
    l2: an 'IwFl' record of metric_type 1 over an 'IxF2' quantizer instead (IndexIVFFlatL2); a metric-0 file is refused by name.
    pq: an 'IwPQ' file instead; the ProductQuantizer record read on the way is appended as (m, codebooks).
    sq: an 'IwSq' file instead; the ScalarQuantizer record's trained values [2d] are appended (QT_8bit), None for QT_fp16."""
    base = f.tell()                                          # (an 'IwPQ' record may sit inside a 'WiPR' file)
    _expect_record(f, p, "IwPQ" if pq else "IwSq" if sq else "IwFl")
    hdr = f.read(_HDR_SIZE + 4)
    d, n, metric, off = _read_header(hdr, 0)
    f.seek(base + 4 + off)
    nlist, nprobe = struct.unpack("<QQ", f.read(16))
    (cq,) = struct.unpack("<I", f.read(4))
    if l2:
        if metric == 0 and cq == _fourcc("IxFI"):
            raise RuntimeError(f"{p}: an IndexIVFFlat file of metric_type 0 (inner product) is not an IndexIVFFlatL2 file; "
                               f"read_ivf_flat_ip reads it")
        if metric != 1 or cq != _fourcc("IxF2"):
            raise RuntimeError(f"{p}: metric_type {metric} over a coarse quantizer of type 0x{cq:08x}: an IndexIVFFlatL2 file has "
                               f"metric_type 1 (METRIC_L2) and an IndexFlatL2 quantizer")
    elif cq != _fourcc("IxFI"):
        raise RuntimeError(f"{p}: coarse quantizer type 0x{cq:08x}, expected IndexFlatIP")
    pos = f.tell()
    hdr = f.read(_HDR_SIZE + 4)
    dq, nq_, qmetric, off = _read_header(hdr, 0)
    if l2 and qmetric != 1:
        raise RuntimeError(f"{p}: the IndexFlatL2 quantizer of an IndexIVFFlatL2 file says metric_type {qmetric}, expected 1")
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
        sq_bytes = {QT_8BIT: d, QT_FP16: 2 * d}.get(qtype)
        if sq_bytes is None or dsq != d or code_size_sq != sq_bytes or cnt != (2 * d if qtype == QT_8BIT else 0):
            raise RuntimeError(f"{p}: unsupported IndexIVFScalarQuantizer (qtype={qtype}, d={dsq}, code_size={code_size_sq}, "
                               f"{cnt} trained values): QT_8bit with one range per dimension is what is read, and qtype 4 "
                               f"(QT_fp16) with no trained value")
        trained = np.fromfile(f, dtype=np.float32, count=cnt)
        code_size_ivf, by_residual = struct.unpack("<QB", f.read(9))
        if trained.size != cnt or code_size_ivf != sq_bytes or by_residual != 1:
            raise RuntimeError(f"{p}: unsupported IndexIVFScalarQuantizer (code_size={code_size_ivf}, by_residual={by_residual})")
        if qtype == QT_FP16:
            trained = None
    il, nl2, code_size = struct.unpack("<IQQ", f.read(20))
    if il != _fourcc("ilar") or nl2 != nlist or code_size != (m if pq else (d if trained is not None else 2 * d) if sq else 4 * d):
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


def read_ivf_flat_ip(path):
    """-> dict(centroids [nlist,d], X [n,d], ids [n], list_off [nlist+1], nprobe).  The lists are returned back to
    back in list order, which is the layout the search kernel wants."""
    p = _existing(path)
    with open(p, "rb") as f:
        centroids, list_off, nprobe, data = _read_ivf_head(f, p)
        X, ids = _read_lists(f, p, list_off, data, centroids.shape[1], np.float32)
    return {"centroids": centroids, "X": X, "ids": ids, "list_off": list_off, "nprobe": nprobe}


def ivf_flat_ip_ntotal(path) -> int:
    """Rows of an 'IwFl' file (its header), without reading the lists."""
    p = _existing(path)
    with open(p, "rb") as f:
        return _record_ntotal(f, p, "IwFl")


def read_ivf_flat_ip_range(path, lo: int, hi: int):
    """Rows [lo, hi) of the list-major array read_ivf_flat_ip returns, reading only the lists that overlap the range
    (one rank's slice of an index sharded across GPUs: wise_amd/index/sharded.py).
    -> dict(centroids [nlist,d] (all of them), X [hi-lo,d], ids [hi-lo], list_off [nlist+1] = clip(list_off - lo, 0,
    hi - lo), nprobe).  List l's payload sits at list_off[l] * (4d + 8) bytes into the payload (rows, then ids)."""
    p = _existing(path)
    with open(p, "rb") as f:
        centroids, list_off, nprobe, data = _read_ivf_head(f, p)
        X, ids, list_off = _read_lists_range(f, p, list_off, data, centroids.shape[1], np.float32, lo, hi, "read_ivf_flat_ip_range")
    return {"centroids": centroids, "X": X, "ids": ids, "list_off": list_off, "nprobe": nprobe}


# ---------------------------------------------------------------------------------------------- 'IwFl', metric_type 1: IndexIVFFlatL2
def write_ivf_flat_l2(path, centroids: np.ndarray, X: np.ndarray, ids: np.ndarray, list_off: np.ndarray, nprobe: int = 1) -> None:
    """faiss's IndexIVFFlat(IndexFlatL2(d), d, nlist, METRIC_L2): the 'IwFl' record of write_ivf_flat_ip with metric_type 1 in its
    header and an 'IxF2' quantizer (metric_type 1) holding the centroids; the raw fp32 rows in the lists, the IP layout otherwise."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    centroids, ids, list_off = _ivf_arrays(centroids, ids, list_off, X.shape[0])
    assert X.shape == (X.shape[0], centroids.shape[1])
    with open(path, "wb") as f:
        _write_ivf_head(f, "IwFl", centroids, X.shape[0], nprobe, metric=1)
        _write_lists(f, X, ids, list_off)


def ivf_flat_metric(path) -> int:
    """metric_type of an 'IwFl' file's header (0: inner product, IndexIVFFlat; 1: L2, IndexIVFFlatL2)."""
    p = _existing(path)
    with open(p, "rb") as f:
        _expect_record(f, p, "IwFl")
        return int(_read_header(f.read(_HDR_SIZE + 4), 0)[2])


def read_ivf_flat_l2(path):
    """-> dict(centroids [nlist,d], X [n,d], ids [n], list_off [nlist+1], nprobe, metric='l2'): read_ivf_flat_ip's dict for an
    IndexIVFFlatL2 file; `metric` is the family's mark.  A metric-0 ('IndexIVFFlat') file is refused by name."""
    p = _existing(path)
    with open(p, "rb") as f:
        centroids, list_off, nprobe, data = _read_ivf_head(f, p, l2=True)
        X, ids = _read_lists(f, p, list_off, data, centroids.shape[1], np.float32)
    return {"centroids": centroids, "X": X, "ids": ids, "list_off": list_off, "nprobe": nprobe, "metric": "l2"}


def ivf_flat_l2_ntotal(path) -> int:
    """Rows of an IndexIVFFlatL2 file (its header), without reading the lists; a metric-0 file is refused as by read_ivf_flat_l2."""
    p = _existing(path)
    with open(p, "rb") as f:
        _, list_off, _, _ = _read_ivf_head(f, p, l2=True)
    return int(list_off[-1])


def read_ivf_flat_l2_range(path, lo: int, hi: int):
    """Rows [lo, hi) of the list-major array read_ivf_flat_l2 returns, reading only the lists that overlap the range: as
    read_ivf_flat_ip_range, with metric='l2'."""
    p = _existing(path)
    with open(p, "rb") as f:
        centroids, list_off, nprobe, data = _read_ivf_head(f, p, l2=True)
        X, ids, list_off = _read_lists_range(f, p, list_off, data, centroids.shape[1], np.float32, lo, hi, "read_ivf_flat_l2_range")
    return {"centroids": centroids, "X": X, "ids": ids, "list_off": list_off, "nprobe": nprobe, "metric": "l2"}


# ---------------------------------------------------------------------------------------------- 'IwPQ': m code bytes a row
def _pq_arrays(centroids, codebooks, codes, ids, list_off):
    codebooks = np.ascontiguousarray(codebooks, dtype=np.float32)
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    n, m = codes.shape
    centroids, ids, list_off = _ivf_arrays(centroids, ids, list_off, n)
    d = centroids.shape[1]
    assert d % m == 0 and codebooks.shape == (m, 256, d // m)
    return centroids, codebooks, codes, ids, list_off


def _refine_arrays(n: int, d: int, kind, k_factor, rows, scales):
    assert kind in (8, 16) and k_factor is not None and k_factor >= 1
    rows = np.ascontiguousarray(rows, dtype=np.int8 if kind == 8 else np.uint16)
    assert rows.shape == (n, d)
    if kind == 8:
        scales = np.ascontiguousarray(scales, dtype=np.float32)
        assert scales.shape == (n,)
    return rows, scales


def write_ivf_pq_ip(path, centroids: np.ndarray, codebooks: np.ndarray, codes: np.ndarray, ids: np.ndarray,
                    list_off: np.ndarray, nprobe: int = 1) -> None:
    """codes [n,m] uint8 / ids hold the lists back to back; codebooks [m,256,d/m] fp32 (8-bit codes, by_residual)."""
    pq = _pq_arrays(centroids, codebooks, codes, ids, list_off)
    with open(path, "wb") as f:
        _write_ivf_pq_record(f, *pq, nprobe)


def _write_ivf_pq_record(f, centroids, codebooks, codes, ids, list_off, nprobe) -> None:
    d, (n, m) = centroids.shape[1], codes.shape
    _write_ivf_head(f, "IwPQ", centroids, n, nprobe)
    f.write(struct.pack("<BQ", 1, m))                        # by_residual, code_size
    f.write(struct.pack("<QQQQ", d, m, 8, 256 * d))          # ProductQuantizer: d, M, nbits, centroids
    codebooks.tofile(f)
    _write_lists(f, codes, ids, list_off)


def _read_ivf_pq_record(f, p):
    centroids, list_off, nprobe, data, m, codebooks = _read_ivf_head(f, p, pq=True)
    codes, ids = _read_lists(f, p, list_off, data, m, np.uint8)
    return {"centroids": centroids, "codebooks": codebooks, "codes": codes, "ids": ids, "list_off": list_off,
            "nprobe": nprobe}


def _read_ivf_pq_record_range(f, p, lo: int, hi: int):
    """Rows [lo, hi) of the list-major arrays of an 'IwPQ' record, reading only the lists that overlap the range.  List l's
    payload sits at list_off[l] * (m + 8) bytes into the payload (codes, then ids).  -> (dict with list_off clipped, n, end of the
    record)."""
    centroids, list_off, nprobe, data, m, codebooks = _read_ivf_head(f, p, pq=True)
    n = int(list_off[-1])
    codes, ids, list_off = _read_lists_range(f, p, list_off, data, m, np.uint8, lo, hi, "read_ivf_pq_ip_range")
    out = {"centroids": centroids, "codebooks": codebooks, "codes": codes, "ids": ids, "list_off": list_off, "nprobe": nprobe}
    return out, n, data + n * (m + 8)


def ivf_pq_ip_ntotal(path) -> int:
    """Rows of an 'IwPQ' file (its header), without reading the lists."""
    p = _existing(path)
    with open(p, "rb") as f:
        return _record_ntotal(f, p, "IwPQ")


def read_ivf_pq_ip_range(path, lo: int, hi: int):
    """Rows [lo, hi) of the list-major arrays read_ivf_pq_ip returns, reading only the lists that overlap the range (one rank's
    slice of an index sharded across GPUs: wise_amd/index/sharded.py).  -> the dict of read_ivf_pq_ip with codes [hi-lo,m],
    ids [hi-lo] and list_off = clip(list_off - lo, 0, hi - lo); centroids and codebooks are whole."""
    p = _existing(path)
    with open(p, "rb") as f:
        return _read_ivf_pq_record_range(f, p, lo, hi)[0]


def read_ivf_pq_ip(path):
    """-> dict(centroids [nlist,d], codebooks [m,256,d/m], codes [n,m] uint8, ids [n], list_off [nlist+1], nprobe), the
    lists back to back in list order."""
    p = _existing(path)
    with open(p, "rb") as f:
        return _read_ivf_pq_record(f, p)


# ---------------------------------------------------------------------------------------------- 'WiPR': a PQ record + compact rows
def _read_refine_head(f, p):
    cc, version, kind, k_factor = struct.unpack("<IIII", f.read(16))
    if cc != _fourcc("WiPR") or version != 1 or kind not in (8, 16) or k_factor < 1:
        raise RuntimeError(f"{p}: not a re-ranking IndexIVFPQ file (type 0x{cc:08x}, version {version}, kind {kind}, "
                           f"k_factor {k_factor})")
    return int(kind), int(k_factor)


def ivf_pq_refine_ip_ntotal(path) -> int:
    """Rows of a 'WiPR' file (the header of its 'IwPQ' record), without reading the lists."""
    p = _existing(path)
    with open(p, "rb") as f:
        _read_refine_head(f, p)
        return _record_ntotal(f, p, "IwPQ")


def read_ivf_pq_refine_ip_range(path, lo: int, hi: int):
    """read_ivf_pq_ip_range for a 'WiPR' file: also rows [lo, hi) of the compact rows and of the scales, read by position (they
    are stored in list order as two plain arrays).  -> the dict of read_ivf_pq_refine_ip over the slice."""
    p = _existing(path)
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


def write_ivf_pq_refine_ip(path, centroids, codebooks, codes, ids, list_off, kind: int, k_factor: int, rows: np.ndarray,
                           scales=None, nprobe: int = 1) -> None:
    """An 'IwPQ' record plus the compact rows of a re-ranking index in the same list order: rows [n,d] int8 with scales [n]
    fp32 (kind 8) or rows [n,d] uint16 bf16 bit patterns (kind 16).  This repository's own format (module docstring)."""
    pq = _pq_arrays(centroids, codebooks, codes, ids, list_off)
    rows, scales = _refine_arrays(pq[2].shape[0], pq[0].shape[1], kind, k_factor, rows, scales)
    with open(path, "wb") as f:
        _write_refine_record(f, *pq, kind, k_factor, rows, scales, nprobe)


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
    p = _existing(path)
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
    pq = _pq_arrays(centroids, codebooks, codes, ids, list_off)
    rotation = np.ascontiguousarray(rotation, dtype=np.float32)
    n, d = pq[2].shape[0], pq[0].shape[1]
    assert rotation.shape == (d, d)
    if kind is not None:
        rows, scales = _refine_arrays(n, d, kind, k_factor, rows, scales)
    with open(path, "wb") as f:
        f.write(struct.pack("<III", _fourcc("WiOP"), 1, d))
        rotation.tofile(f)
        if kind is None:
            _write_ivf_pq_record(f, *pq, nprobe)
        else:
            _write_refine_record(f, *pq, kind, k_factor, rows, scales, nprobe)


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
    p = _existing(path)
    with open(p, "rb") as f:
        rotation, inner = _read_opq_head(f, p)
        return _with_rotation(_read_ivf_pq_record(f, p) if inner == _fourcc("IwPQ") else _read_refine_record(f, p), rotation, p)


def ivf_opq_ip_ntotal(path) -> int:
    """Rows of a 'WiOP' file (the header of its 'IwPQ' record), without reading the lists."""
    p = _existing(path)
    with open(p, "rb") as f:
        _, inner = _read_opq_head(f, p)
        if inner == _fourcc("WiPR"):
            _read_refine_head(f, p)
        return _record_ntotal(f, p, "IwPQ")


def read_ivf_opq_ip_range(path, lo: int, hi: int):
    """Rows [lo, hi) of the list-major arrays read_ivf_opq_ip returns, as read_ivf_pq_ip_range / read_ivf_pq_refine_ip_range cut them
    out of the wrapped record; the rotation is whole."""
    p = _existing(path)
    with open(p, "rb") as f:
        rotation, inner = _read_opq_head(f, p)
        out = _read_ivf_pq_record_range(f, p, lo, hi)[0] if inner == _fourcc("IwPQ") else _read_refine_record_range(f, p, lo, hi)
        return _with_rotation(out, rotation, p)


# ---------------------------------------------------------------------------------------------- 'IwSq': 8-bit scalar quantizer
def write_ivf_sq_ip(path, centroids: np.ndarray, trained: np.ndarray, codes: np.ndarray, ids: np.ndarray, list_off: np.ndarray,
                    nprobe: int = 1) -> None:
    """codes [n,d] uint8 / ids hold the lists back to back; trained [2d] fp32 = vmin, then vdiff (QT_8bit, by_residual)."""
    trained = np.ascontiguousarray(trained, dtype=np.float32)
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    n = codes.shape[0]
    centroids, ids, list_off = _ivf_arrays(centroids, ids, list_off, n)
    d = centroids.shape[1]
    assert codes.shape == (n, d) and trained.shape == (2 * d,)
    with open(path, "wb") as f:
        _write_ivf_head(f, "IwSq", centroids, n, nprobe)
        f.write(struct.pack("<iifQQ", QT_8BIT, 0, 0.0, d, d))          # ScalarQuantizer: qtype, rangestat, rangestat_arg, d, code_size
        f.write(struct.pack("<Q", 2 * d))
        trained.tofile(f)
        f.write(struct.pack("<QB", d, 1))                        # code_size, by_residual
        _write_lists(f, codes, ids, list_off)


def write_ivf_sq16_ip(path, centroids: np.ndarray, halves: np.ndarray, ids: np.ndarray, list_off: np.ndarray, nprobe: int = 1) -> None:
    """halves [n,d] float16 / ids hold the lists back to back (QT_fp16, by_residual: nothing trained)."""
    halves = np.ascontiguousarray(halves, dtype="<f2")
    n = halves.shape[0]
    centroids, ids, list_off = _ivf_arrays(centroids, ids, list_off, n)
    d = centroids.shape[1]
    assert halves.shape == (n, d)
    with open(path, "wb") as f:
        _write_ivf_head(f, "IwSq", centroids, n, nprobe)
        f.write(struct.pack("<iifQQ", QT_FP16, 0, 0.0, d, 2 * d))      # ScalarQuantizer: qtype, rangestat, rangestat_arg, d, code_size
        f.write(struct.pack("<Q", 0))                            # trained: empty
        f.write(struct.pack("<QB", 2 * d, 1))                    # code_size, by_residual
        _write_lists(f, halves, ids, list_off)


def _sq_state(centroids, trained, payload, ids, list_off, nprobe) -> dict:
    """the dict of the 'IwSq' readers: 'trained' and 'codes' (QT_8bit), or 'halves' alone (QT_fp16: trained is None)"""
    if trained is None:
        return {"centroids": centroids, "halves": payload, "ids": ids, "list_off": list_off, "nprobe": nprobe}
    return {"centroids": centroids, "trained": trained, "codes": payload, "ids": ids, "list_off": list_off, "nprobe": nprobe}


def _read_ivf_sq_head(f, p):
    try:
        return _read_ivf_head(f, p, sq=True)
    except (struct.error, ValueError) as e:
        raise RuntimeError(f"{p}: the head of an IndexIVFScalarQuantizer file is cut short ({e})") from None


def read_ivf_sq_ip(path):
    """-> dict(centroids [nlist,d], trained [2d] (vmin, then vdiff), codes [n,d] uint8, ids [n], list_off [nlist+1], nprobe), the
    lists back to back in list order; for a QT_fp16 file dict(centroids, halves [n,d] float16, ids, list_off, nprobe).  A file cut
    short is refused (RuntimeError)."""
    p = _existing(path)
    with open(p, "rb") as f:
        centroids, list_off, nprobe, data, trained = _read_ivf_sq_head(f, p)
        payload, ids = _read_lists(f, p, list_off, data, centroids.shape[1], np.uint8 if trained is not None else np.dtype("<f2"),
                                   strict=True)
    return _sq_state(centroids, trained, payload, ids, list_off, nprobe)


def ivf_sq_ip_ntotal(path) -> int:
    """Rows of an 'IwSq' file (its header), without reading the lists."""
    p = _existing(path)
    with open(p, "rb") as f:
        return _record_ntotal(f, p, "IwSq")


def read_ivf_sq_ip_range(path, lo: int, hi: int):
    """Rows [lo, hi) of the list-major arrays read_ivf_sq_ip returns, reading only the lists that overlap the range (one rank's
    slice of an index sharded across GPUs: wise_amd/index/sharded.py).  -> the dict of read_ivf_sq_ip with codes [hi-lo,d],
    ids [hi-lo] and list_off = clip(list_off - lo, 0, hi - lo); centroids and trained are whole.  List l's payload sits at
    list_off[l] * (d + 8) bytes into the payload (codes, then ids); 2d + 8 and 'halves' for a QT_fp16 file."""
    p = _existing(path)
    with open(p, "rb") as f:
        centroids, list_off, nprobe, data, trained = _read_ivf_sq_head(f, p)
        payload, ids, list_off = _read_lists_range(f, p, list_off, data, centroids.shape[1],
                                                   np.uint8 if trained is not None else np.dtype("<f2"), lo, hi, "read_ivf_sq_ip_range",
                                                   strict=True)
    return _sq_state(centroids, trained, payload, ids, list_off, nprobe)


def index_fourcc(path, inner: bool = False) -> str:
    """The fourcc the file opens with; inner: for an 'IxMp' (IndexIDMap) file the fourcc of the index it wraps — 'IxFI' for
    IndexFlatIP, 'IxF2' for IndexFlatL2, 'IxSQ' for IndexSQfp16, 'IxPq' for IndexPQ<m> — ('' where the file ends before it), for any
    other file its own ('WiFR' for IndexPQ<m>R8 / R16)."""
    with open(path, "rb") as f:
        head = f.read(_FLAT_HEAD_BYTES if inner else 4)
    if not inner or head[:4] != b"IxMp":
        return head[:4].decode("ascii", errors="replace")
    try:
        return struct.pack("<I", _flat_outer(head)[1]).decode("ascii", errors="replace")
    except struct.error:
        return ""


# ---------------------------------------------------------------------------------------------- 'IxMp' around 'IxSQ': binary16 rows
def write_idmap_sq16_ip(path, halves: np.ndarray, ids: np.ndarray) -> None:
    """halves [n,d] float16 (IEEE binary16), ids [n] int64: IndexIDMap around IndexScalarQuantizer(d, QT_fp16, inner product)."""
    _write_idmap_sq16(path, halves, ids, 0)


def _write_idmap_sq16(path, halves, ids, metric: int) -> None:
    """the QT_fp16 'IxSQ' file under either metric_type (0: IndexSQfp16, 1: IndexSQfp16L2), written into both headers"""
    halves = np.ascontiguousarray(halves, dtype="<f2")
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    n, d = halves.shape
    assert ids.shape == (n,)
    with open(path, "wb") as f:
        f.write(struct.pack("<I", _fourcc("IxMp")))
        f.write(_header(d, n, metric))
        f.write(struct.pack("<I", _fourcc("IxSQ")))
        f.write(_header(d, n, metric))
        f.write(struct.pack("<iifQQ", QT_FP16, 0, 0.0, d, 2 * d))      # ScalarQuantizer: qtype, rangestat, rangestat_arg, d, code_size
        f.write(struct.pack("<Q", 0))                            # trained: empty
        f.write(struct.pack("<Q", n * 2 * d))                    # codes
        halves.tofile(f)
        f.write(struct.pack("<Q", n))
        ids.tofile(f)


def read_idmap_sq16_ip(path, mmap: bool = True):
    """-> (halves [n,d] float16 (a memmap view unless mmap is False), ids int64[n]) of an IndexSQfp16 file; a bare 'IxSQ' file
    (no id map) gives ids = positions.  RuntimeError naming the file for a missing, truncated or foreign file."""
    p = _existing(path)
    head = _flat_head(p, "IxSQ", sq_metric=0)
    return _flat_rows(p, head, mmap), _flat_ids(p, head, 0, head.n)


def read_idmap_sq16_ip_range(path, lo: int, hi: int):
    """Rows [lo, hi) of what read_idmap_sq16_ip returns, reading only those rows and ids (one rank's shard_range of the file)."""
    p = _existing(path)
    head = _flat_head(p, "IxSQ", sq_metric=0)
    lo, hi = int(lo), int(hi)
    if not (0 <= lo <= hi <= head.n):
        raise ValueError(f"read_idmap_sq16_ip_range: [{lo}, {hi}) outside [0, {head.n}]")
    H = np.fromfile(p, dtype=head.dtype, count=(hi - lo) * head.d, offset=head.off + lo * 2 * head.d).reshape(hi - lo, head.d)
    return H, _flat_ids(p, head, lo, hi)


def idmap_sq16_ip_ntotal(path) -> int:
    """Rows of an IndexSQfp16 file (its header)."""
    return _flat_head(_existing(path), "IxSQ", sq_metric=0).n


def write_idmap_sq16_l2(path, halves: np.ndarray, ids: np.ndarray) -> None:
    """halves [n,d] float16 (IEEE binary16), ids [n] int64: IndexIDMap around IndexScalarQuantizer(d, QT_fp16, METRIC_L2) — the
    IndexSQfp16 layout with metric_type 1 in both headers."""
    _write_idmap_sq16(path, halves, ids, 1)


def read_idmap_sq16_l2(path, mmap: bool = True):
    """-> (halves [n,d] float16 (a memmap view unless mmap is False), ids int64[n]) of an IndexSQfp16L2 file; a bare 'IxSQ' file
    (no id map) gives ids = positions.  RuntimeError naming the file for a missing, truncated or foreign file — an IndexSQfp16 file
    (metric_type 0) among them, by name."""
    p = _existing(path)
    head = _flat_head(p, "IxSQ", sq_metric=1)
    return _flat_rows(p, head, mmap), _flat_ids(p, head, 0, head.n)


def read_idmap_sq16_l2_range(path, lo: int, hi: int):
    """Rows [lo, hi) of what read_idmap_sq16_l2 returns, reading only those rows and ids (one rank's shard_range of the file)."""
    p = _existing(path)
    head = _flat_head(p, "IxSQ", sq_metric=1)
    lo, hi = int(lo), int(hi)
    if not (0 <= lo <= hi <= head.n):
        raise ValueError(f"read_idmap_sq16_l2_range: [{lo}, {hi}) outside [0, {head.n}]")
    H = np.fromfile(p, dtype=head.dtype, count=(hi - lo) * head.d, offset=head.off + lo * 2 * head.d).reshape(hi - lo, head.d)
    return H, _flat_ids(p, head, lo, hi)


def idmap_sq16_l2_ntotal(path) -> int:
    """Rows of an IndexSQfp16L2 file (its header)."""
    return _flat_head(_existing(path), "IxSQ", sq_metric=1).n


def flat_sq_metric(path):
    """metric_type of the 'IxSQ' record of a file, bare or inside 'IxMp' (0: inner product, 1: L2 — what tells an IndexSQfp16L2 file
    from an IndexSQfp16 one, as ivf_flat_metric tells the two 'IwFl' files apart); None where the file is no such file or ends before
    it."""
    with open(path, "rb") as f:
        head = f.read(_FLAT_HEAD_BYTES)
    try:
        _, inner, off, _, _ = _flat_outer(head)
        if inner != _fourcc("IxSQ"):
            return None
        return _read_header(head, off)[2]
    except struct.error:
        return None


def _read_sq16_state(path):
    H, ids = read_idmap_sq16_ip(path, mmap=False)
    return {"halves": H, "ids": ids}


def _read_sq16_state_range(path, lo, hi):
    H, ids = read_idmap_sq16_ip_range(path, lo, hi)
    return {"halves": H, "ids": ids}


# ---------------------------------------------------------------------------------------------- 'IxMp' around 'IxSQ': 8-bit codes
def write_idmap_sq8_ip(path, trained: np.ndarray, codes: np.ndarray, ids: np.ndarray) -> None:
    """trained [2d] float32 (vmin, then vdiff), codes [n,d] uint8, ids [n] int64: IndexIDMap around IndexScalarQuantizer(d, QT_8bit,
    inner product) with RS_minmax, argument 0 — faiss's layout of index type 'IndexSQ8bit'."""
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    trained = np.ascontiguousarray(trained, dtype="<f4").reshape(-1)
    n, d = codes.shape
    assert ids.shape == (n,) and trained.shape == (2 * d,)
    with open(path, "wb") as f:
        f.write(struct.pack("<I", _fourcc("IxMp")))
        f.write(_header(d, n))
        f.write(struct.pack("<I", _fourcc("IxSQ")))
        f.write(_header(d, n))
        f.write(struct.pack("<iifQQ", QT_8BIT, 0, 0.0, d, d))          # ScalarQuantizer: qtype, rangestat, rangestat_arg, d, code_size
        f.write(struct.pack("<Q", 2 * d))
        trained.tofile(f)
        f.write(struct.pack("<Q", n * d))                        # codes
        codes.tofile(f)
        f.write(struct.pack("<Q", n))
        ids.tofile(f)


def read_idmap_sq8_ip(path, mmap: bool = True):
    """-> (trained [2d] float32, codes [n,d] uint8 (a memmap view unless mmap is False), ids int64[n]) of an IndexSQ8bit file; a bare
    'IxSQ' file (no id map) gives ids = positions.  RuntimeError naming the file for a missing, truncated or foreign file — an
    IndexSQfp16 file (qtype 4) among them."""
    p = _existing(path)
    head = _flat_head(p, "IxSQ", QT_8BIT)
    return head.trained, _flat_rows(p, head, mmap), _flat_ids(p, head, 0, head.n)


def read_idmap_sq8_ip_range(path, lo: int, hi: int):
    """(trained, codes, ids) with rows [lo, hi) of what read_idmap_sq8_ip returns, reading only those rows and ids (one rank's
    shard_range of the file); the ranges are whole."""
    p = _existing(path)
    head = _flat_head(p, "IxSQ", QT_8BIT)
    lo, hi = int(lo), int(hi)
    if not (0 <= lo <= hi <= head.n):
        raise ValueError(f"read_idmap_sq8_ip_range: [{lo}, {hi}) outside [0, {head.n}]")
    C = np.fromfile(p, dtype=np.uint8, count=(hi - lo) * head.d, offset=head.off + lo * head.d).reshape(hi - lo, head.d)
    return head.trained, C, _flat_ids(p, head, lo, hi)


def idmap_sq8_ip_ntotal(path) -> int:
    """Rows of an IndexSQ8bit file (its header)."""
    return _flat_head(_existing(path), "IxSQ", QT_8BIT).n


def flat_sq_qtype(path):
    """qtype of the ScalarQuantizer record of an 'IxSQ' file, bare or inside 'IxMp' (0: IndexSQ8bit, 4: IndexSQfp16); None where the
    file is no such file or ends before it."""
    with open(path, "rb") as f:
        head = f.read(_FLAT_HEAD_BYTES)
    try:
        _, inner, off, _, _ = _flat_outer(head)
        if inner != _fourcc("IxSQ"):
            return None
        _, _, _, off = _read_header(head, off)
        return struct.unpack_from("<i", head, off)[0]
    except struct.error:
        return None


def _read_sq8_state(path):
    trained, C, ids = read_idmap_sq8_ip(path, mmap=False)
    return {"trained": trained, "codes": C, "ids": ids}


def _read_sq8_state_range(path, lo, hi):
    trained, C, ids = read_idmap_sq8_ip_range(path, lo, hi)
    return {"trained": trained, "codes": C, "ids": ids}


# ---------------------------------------------------------------------------------------------- 'IxMp' around 'IxPq': m code bytes a row, no lists
def _pq_flat_arrays(codebooks, codes, ids):
    codebooks = np.ascontiguousarray(codebooks, dtype="<f4")
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    assert codes.ndim == 2 and codebooks.ndim == 3
    n, m = codes.shape
    assert ids.shape == (n,) and codebooks.shape[:2] == (m, 256) and codebooks.shape[2] >= 1
    return codebooks, codes, ids


def _write_idmap_pq_record(f, codebooks, codes, ids) -> None:
    (n, m), d = codes.shape, codebooks.shape[0] * codebooks.shape[2]
    f.write(struct.pack("<I", _fourcc("IxMp")))
    f.write(_header(d, n))
    f.write(struct.pack("<I", _fourcc("IxPq")))
    f.write(_header(d, n))
    f.write(struct.pack("<QQQQ", d, m, 8, 256 * d))          # ProductQuantizer: d, M, nbits, centroids
    codebooks.tofile(f)
    f.write(struct.pack("<Q", n * m))                        # codes
    codes.tofile(f)
    f.write(struct.pack("<iBi", 0, 0, 8 * m + 1))            # search_type ST_PQ, encode_signs, polysemous_ht
    f.write(struct.pack("<Q", n))
    ids.tofile(f)


def write_idmap_pq_ip(path, codebooks: np.ndarray, codes: np.ndarray, ids: np.ndarray) -> None:
    """codebooks [m,256,d/m] float32, codes [n,m] uint8, ids [n] int64: IndexIDMap around IndexPQ(d, m, 8, inner product) — faiss's
    layout of index types 'IndexPQ<m>'."""
    with open(path, "wb") as f:
        _write_idmap_pq_record(f, *_pq_flat_arrays(codebooks, codes, ids))


class _PQFlatHead(NamedTuple):
    """The head of an 'IxPq' record, bare or inside 'IxMp' (_pq_flat_head); offsets are absolute."""
    d: int
    m: int
    n: int
    codebooks: np.ndarray
    off: int             # of the codes
    idmap: bool
    end: int             # of the record


_PQ_TAIL = struct.calcsize("<iBi")


def _pq_flat_head(f, p, size: int) -> _PQFlatHead:
    """Parse the 'IxPq' record the open file stands at, up to its codes; RuntimeError naming the file for anything else or a record
    that contradicts itself or ends early."""
    base = f.tell()
    try:
        head = f.read(4 + (_HDR_SIZE + 4) + 4 + (_HDR_SIZE + 4))
        cc, inner, off, d0, n0 = _flat_outer(head)
        idmap = cc == _fourcc("IxMp")
        if inner != _fourcc("IxPq"):
            raise RuntimeError(f"{p}: index type 0x{inner:08x} is not IndexPQ ('IxPq', bare or inside 'IxMp')")
        d, n, metric, off = _read_header(head, off)
        f.seek(base + off)
        dp, m, nbits, cnt = struct.unpack("<QQQQ", f.read(32))
    except struct.error as e:
        raise RuntimeError(f"{p}: the head of an IndexPQ file is cut short ({e})") from None
    if metric != 0 or (idmap and struct.unpack_from("<i", head, 4 + _HDR_SIZE - 4)[0] != 0):
        raise RuntimeError(f"{p}: an IndexPQ file with metric_type {metric}: inner product (metric_type 0) is what is read")
    if nbits != 8 or d < 1 or dp != d or m < 1 or m > d or d % m or cnt != 256 * d or n < 0 or (idmap and (d0 != d or n0 != n)):
        raise RuntimeError(f"{p}: unsupported IndexPQ (d={dp} under a header of d={d}, M={m}, nbits={nbits}, {cnt} codebook values, "
                           f"{n} rows): 8-bit codes with 256 d codebook values are what is read")
    codebooks = np.fromfile(f, dtype="<f4", count=int(cnt))
    tail = f.read(8)
    if codebooks.size != cnt or len(tail) != 8:
        raise RuntimeError(f"{p}: the codebooks of an IndexPQ file are cut short")
    (nbytes,) = struct.unpack("<Q", tail)
    if nbytes != n * m:
        raise RuntimeError(f"{p}: {nbytes} code bytes for {n} x {m} 8-bit codes")
    off = f.tell()
    end = off + n * m + _PQ_TAIL + ((8 + 8 * n) if idmap else 0)
    if size < end:
        raise RuntimeError(f"{p}: the file is cut short ({size} bytes, {end} promised by its header)")
    return _PQFlatHead(int(d), int(m), int(n), codebooks.astype(np.float32).reshape(m, 256, d // m), int(off), idmap, int(end))


def _pq_flat_ids(f, p, head: _PQFlatHead, lo: int, hi: int):
    if not head.idmap:
        return np.arange(lo, hi, dtype=np.int64)
    f.seek(head.off + head.n * head.m + _PQ_TAIL)
    (nid,) = struct.unpack("<Q", f.read(8))
    if nid != head.n:
        raise RuntimeError(f"{p}: id_map has {nid} entries for {head.n} rows")
    f.seek(8 * lo, 1)
    ids = np.fromfile(f, dtype=np.int64, count=hi - lo)
    if ids.size != hi - lo:
        raise RuntimeError(f"{p}: the id_map is cut short ({ids.size} of {hi - lo} ids)")
    return ids


def _read_idmap_pq_record(f, p, lo=None, hi=None, mmap: bool = True, who: str = "read_idmap_pq_ip_range"):
    """(dict(codebooks, codes, ids) of rows [lo, hi) — default all, the codes then a memmap view unless mmap is False —, the head)
    of the 'IxPq' record the open file stands at."""
    head = _pq_flat_head(f, p, p.stat().st_size)
    whole = lo is None
    lo, hi = (0, head.n) if whole else (int(lo), int(hi))
    if not (0 <= lo <= hi <= head.n):
        raise ValueError(f"{who}: [{lo}, {hi}) outside [0, {head.n}]")
    if whole and mmap and head.n:
        codes = np.memmap(p, dtype=np.uint8, mode="r", offset=head.off, shape=(head.n, head.m))
    else:
        codes = np.fromfile(p, dtype=np.uint8, count=(hi - lo) * head.m, offset=head.off + lo * head.m).reshape(hi - lo, head.m)
    return {"codebooks": head.codebooks, "codes": codes, "ids": _pq_flat_ids(f, p, head, lo, hi)}, head


def read_idmap_pq_ip(path, mmap: bool = True):
    """-> dict(codebooks [m,256,d/m] float32, codes [n,m] uint8 (a memmap view unless mmap is False), ids int64[n]) of an IndexPQ<m>
    file; a bare 'IxPq' file (no id map) gives ids = positions.  RuntimeError naming the file for a missing, truncated, foreign or
    self-contradicting file."""
    p = _existing(path)
    with open(p, "rb") as f:
        return _read_idmap_pq_record(f, p, mmap=mmap)[0]


def read_idmap_pq_ip_range(path, lo: int, hi: int):
    """Rows [lo, hi) of what read_idmap_pq_ip returns, reading only those codes and ids; the codebooks are whole."""
    p = _existing(path)
    with open(p, "rb") as f:
        return _read_idmap_pq_record(f, p, lo, hi)[0]


def idmap_pq_ip_ntotal(path) -> int:
    """Rows of an IndexPQ<m> file (its header)."""
    p = _existing(path)
    with open(p, "rb") as f:
        return _pq_flat_head(f, p, p.stat().st_size).n


# ---------------------------------------------------------------------------------------------- 'WiFR': an 'IxPq' record + compact rows
def write_pq_refine_ip(path, codebooks, codes, ids, kind: int, k_factor: int, rows: np.ndarray, scales=None) -> None:
    """The 'IxMp' / 'IxPq' record plus the compact rows of a re-ranking index in the same row order: rows [n,d] int8 with scales [n]
    fp32 (kind 8) or rows [n,d] uint16 bf16 bit patterns (kind 16).  This repository's own format (module docstring)."""
    codebooks, codes, ids = _pq_flat_arrays(codebooks, codes, ids)
    rows, scales = _refine_arrays(codes.shape[0], codebooks.shape[0] * codebooks.shape[2], kind, k_factor, rows, scales)
    with open(path, "wb") as f:
        f.write(struct.pack("<IIII", _fourcc("WiFR"), 1, kind, k_factor))
        _write_idmap_pq_record(f, codebooks, codes, ids)
        f.write(struct.pack("<Q", rows.nbytes))
        rows.tofile(f)
        if kind == 8:
            f.write(struct.pack("<Q", rows.shape[0]))
            scales.tofile(f)


def _read_pq_refine_head(f, p):
    head = f.read(16)
    if len(head) != 16:
        raise RuntimeError(f"{p}: the head of a re-ranking IndexPQ file is cut short")
    cc, version, kind, k_factor = struct.unpack("<IIII", head)
    if cc != _fourcc("WiFR") or version != 1 or kind not in (8, 16) or k_factor < 1:
        raise RuntimeError(f"{p}: not a re-ranking IndexPQ file (type 0x{cc:08x}, version {version}, kind {kind}, k_factor {k_factor})")
    return int(kind), int(k_factor)


def _read_pq_refine(path, lo=None, hi=None, mmap: bool = True):
    p = _existing(path)
    size = p.stat().st_size
    with open(p, "rb") as f:
        kind, k_factor = _read_pq_refine_head(f, p)
        out, head = _read_idmap_pq_record(f, p, lo, hi, mmap, "read_pq_refine_ip_range")
        lo, hi = (0, head.n) if lo is None else (int(lo), int(hi))
        n, d = head.n, head.d
        width = d * (1 if kind == 8 else 2)
        if size < head.end + 8 + n * width + ((8 + 4 * n) if kind == 8 else 0):
            raise RuntimeError(f"{p}: the file is cut short ({size} bytes: the compact rows of {n} x {d} of kind {kind} do not fit)")
        f.seek(head.end)
        (nbytes,) = struct.unpack("<Q", f.read(8))
        if nbytes != n * width:
            raise RuntimeError(f"{p}: {nbytes} bytes of compact rows for {n} x {d} of kind {kind}")
        f.seek(head.end + 8 + lo * width)
        rows = np.fromfile(f, dtype=np.int8 if kind == 8 else np.uint16, count=(hi - lo) * d).reshape(hi - lo, d)
        scales = None
        if kind == 8:
            f.seek(head.end + 8 + n * width)
            (ns,) = struct.unpack("<Q", f.read(8))
            if ns != n:
                raise RuntimeError(f"{p}: {ns} scales for {n} rows")
            f.seek(4 * lo, 1)
            scales = np.fromfile(f, dtype=np.float32, count=hi - lo)
    out.update(kind=kind, k_factor=k_factor, rows=rows, scales=scales)
    return out


def read_pq_refine_ip(path, mmap: bool = True):
    """-> the dict of read_idmap_pq_ip plus kind, k_factor, rows [n,d] (int8 / uint16 bf16 bits) and scales [n] (None for kind 16)."""
    return _read_pq_refine(path, mmap=mmap)


def read_pq_refine_ip_range(path, lo: int, hi: int):
    """Rows [lo, hi) of what read_pq_refine_ip returns, read by position; the codebooks are whole."""
    return _read_pq_refine(path, lo, hi)


def pq_refine_ip_ntotal(path) -> int:
    """Rows of a 'WiFR' file (the header of its 'IxPq' record)."""
    p = _existing(path)
    with open(p, "rb") as f:
        _read_pq_refine_head(f, p)
        return _pq_flat_head(f, p, p.stat().st_size).n


# ---------------------------------------------------------------------------------------------- any IVF file, by its fourcc
_BY_FOURCC = {                                    # fourcc -> (reader, range reader, ntotal)
    "IwFl": (read_ivf_flat_ip, read_ivf_flat_ip_range, ivf_flat_ip_ntotal),
    "IwFl/L2": (read_ivf_flat_l2, read_ivf_flat_l2_range, ivf_flat_l2_ntotal),   # the record's metric_type 1: IndexIVFFlatL2
    "IwPQ": (read_ivf_pq_ip, read_ivf_pq_ip_range, ivf_pq_ip_ntotal),
    "WiPR": (read_ivf_pq_refine_ip, read_ivf_pq_refine_ip_range, ivf_pq_refine_ip_ntotal),
    "WiOP": (read_ivf_opq_ip, read_ivf_opq_ip_range, ivf_opq_ip_ntotal),
    "IwSq": (read_ivf_sq_ip, read_ivf_sq_ip_range, ivf_sq_ip_ntotal),
    "IxSQ": (_read_sq16_state, _read_sq16_state_range, idmap_sq16_ip_ntotal),      # IndexSQfp16: no lists, dict(halves, ids)
    "IxSQ/L2": (lambda path: dict(zip(("halves", "ids"), read_idmap_sq16_l2(path, mmap=False)), metric="l2"),
                lambda path, lo, hi: dict(zip(("halves", "ids"), read_idmap_sq16_l2_range(path, lo, hi)), metric="l2"),
                idmap_sq16_l2_ntotal),                                             # IndexSQfp16L2: the same with metric_type 1
    "IxSQ/8": (_read_sq8_state, _read_sq8_state_range, idmap_sq8_ip_ntotal),      # IndexSQ8bit: no lists, dict(trained, codes, ids)
}
_BY_FOURCC_PQ_FLAT = {                            # the list-less product-quantizer files: dict(codebooks, codes, ids[, kind, ...])
    "IxPq": (read_idmap_pq_ip, read_idmap_pq_ip_range, idmap_pq_ip_ntotal),
    "WiFR": (read_pq_refine_ip, read_pq_refine_ip_range, pq_refine_ip_ntotal),
}


def _by_fourcc(path, which: int):
    p = _existing(path)
    cc = index_fourcc(p)
    if cc == "IxMp" and index_fourcc(p, inner=True) == "IxSQ":
        cc = "IxSQ"
    if cc == "IxMp" and index_fourcc(p, inner=True) == "IxPq":
        cc = "IxPq"
    if cc in _BY_FOURCC_PQ_FLAT:
        return _BY_FOURCC_PQ_FLAT[cc][which]
    if cc == "IxSQ" and flat_sq_qtype(p) == QT_8BIT:         # the record's qtype tells the two 'IxSQ' files apart
        cc = "IxSQ/8"
    if cc == "IxSQ" and flat_sq_metric(p) == 1:              # the record's metric_type tells the two QT_fp16 'IxSQ' files apart
        cc = "IxSQ/L2"
    if cc == "IwFl" and ivf_flat_metric(p) == 1:             # the record's metric_type tells the two 'IwFl' files apart
        cc = "IwFl/L2"
    if cc not in _BY_FOURCC:
        names = ', '.join(k for k in _BY_FOURCC if not k.startswith('IxSQ') and '/' not in k)
        raise RuntimeError(f"{p}: index type {cc!r} is not an inverted-file index ({names}) "
                           f"nor an IndexSQfp16 file ('IxSQ', bare or inside 'IxMp') nor an IndexSQ8bit file (the same with qtype 0)")
    return _BY_FOURCC[cc][which]


def read_index(path):
    """The dict of the named reader of the file's record: read_ivf_flat_ip ('IwFl'; read_ivf_flat_l2 where the record's metric_type is
    1), read_ivf_pq_ip ('IwPQ'), read_ivf_pq_refine_ip
    ('WiPR'), read_ivf_opq_ip ('WiOP') or read_ivf_sq_ip ('IwSq').  (The flat 'IxMp' file holds no lists: read_idmap_flat_ip.)"""
    return _by_fourcc(path, 0)(path)


def read_index_range(path, lo: int, hi: int):
    """Rows [lo, hi) of the list-major arrays read_index returns, by the range reader of the file's record."""
    return _by_fourcc(path, 1)(path, lo, hi)


def index_ntotal(path) -> int:
    """Rows of an IVF file of any record (its header), without reading the lists."""
    return _by_fourcc(path, 2)(path)


def write_index(path, state, nprobe=None) -> None:
    """The inverse of read_index: `state` is a dict with a reader's keys, and the keys pick the record — 'rotation': 'WiOP'; else
    'kind': 'WiPR'; else 'codebooks': 'IwPQ'; else 'trained': 'IwSq'; else 'halves': 'IwSq' with QT_fp16; else 'X': 'IwFl' (with
    metric == 'l2': its metric_type 1 form); 'halves'
    without 'centroids' is the list-less IndexSQfp16 file ('IxMp' around 'IxSQ'), 'trained' without 'centroids' the IndexSQ8bit file,
    'codebooks' without 'centroids' the IndexPQ<m> file ('IxMp' around 'IxPq'; with 'kind' its 'WiFR' form).  nprobe: state's own unless given."""
    if "halves" in state and "centroids" not in state:       # IndexSQfp16 (with metric == 'l2': IndexSQfp16L2): rows and ids, no lists
        return (write_idmap_sq16_l2 if state.get("metric") == "l2" else write_idmap_sq16_ip)(path, state["halves"], state["ids"])
    if "trained" in state and "centroids" not in state:      # IndexSQ8bit: ranges, codes and ids, no lists
        return write_idmap_sq8_ip(path, state["trained"], state["codes"], state["ids"])
    if "codebooks" in state and "centroids" not in state:    # IndexPQ<m> (with 'kind': its R8 / R16 form): codebooks, codes and ids, no lists
        if "kind" in state:
            return write_pq_refine_ip(path, state["codebooks"], state["codes"], state["ids"], state["kind"], state["k_factor"],
                                      state["rows"], state.get("scales"))
        return write_idmap_pq_ip(path, state["codebooks"], state["codes"], state["ids"])
    nprobe = state.get("nprobe", 1) if nprobe is None else nprobe
    lists = (state["ids"], state["list_off"])
    store = {k: state[k] for k in ("kind", "k_factor", "rows", "scales") if k in state}
    if "rotation" in state:
        write_ivf_opq_ip(path, state["rotation"], state["centroids"], state["codebooks"], state["codes"], *lists, nprobe=nprobe, **store)
    elif "kind" in state:
        write_ivf_pq_refine_ip(path, state["centroids"], state["codebooks"], state["codes"], *lists, nprobe=nprobe, **store)
    elif "codebooks" in state:
        write_ivf_pq_ip(path, state["centroids"], state["codebooks"], state["codes"], *lists, nprobe=nprobe)
    elif "trained" in state:
        write_ivf_sq_ip(path, state["centroids"], state["trained"], state["codes"], *lists, nprobe=nprobe)
    elif "halves" in state:
        write_ivf_sq16_ip(path, state["centroids"], state["halves"], *lists, nprobe=nprobe)
    elif "X" in state and state.get("metric") == "l2":       # IndexIVFFlatL2: the 'IwFl' record with metric_type 1
        write_ivf_flat_l2(path, state["centroids"], state["X"], *lists, nprobe=nprobe)
    elif "X" in state:
        write_ivf_flat_ip(path, state["centroids"], state["X"], *lists, nprobe=nprobe)
    else:
        raise TypeError(f"write_index: no record for a state of {sorted(state)}")
