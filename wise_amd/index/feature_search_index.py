"""FeatureSearchIndex — the reference's plugin boundary for vector search (src/index/feature_search_index.py:13-114)
over an index resident in HBM and searched by the HIP scan+top-k kernels.

`__init__`, `get_index_filename`, `is_index_loaded` and `search` are restated VERBATIM from
src/index/feature_search_index.py:14-31, :87-88 and :100-114 — they ARE the boundary, and their quirks are part of
the contract a drop-in must keep (the prompt rules, the missing `f` prefix in the
`query_type` error message, the 1-D return of the first query only).  `create_index` and `load_index` are new:
they build / read the same `.faiss` files without faiss (wise_amd/index/faiss_io.py) into FlatIPIndex / IVFFlatIPIndex.

Same constructor contract (asserts on 'features_dir'/'index_dir'), prompts, file naming
(`{index_dir}/{media_type}-{index_type}.faiss`), skip-if-exists create, `load_index` that also
builds the FeatureExtractor, and the prompt quirks of `search`.  Both index types the
reference offers are built: `IndexFlatIP` (exhaustive, the hot path) and `IndexIVFFlat` (approximate; cell count
and training-sample size chosen as at feature_search_index.py:55-59, k-means and list scan on the GPU).  A third,
`IndexIVFPQ<m>` (for example `IndexIVFPQ64`; bare `IndexIVFPQ` = m = d / 4), is the IVF+PQ family of the reference's index
study (docs/Search-Index-Evaluation.md:105-123): the same coarse stage over lists of m-byte codes (wise_amd/index/ivf_pq.py).
`IndexIVFPQ<m>R8` / `IndexIVFPQ<m>R16` (for example `IndexIVFPQ64R8`) are that index with a re-ranking stage over compact rows kept
beside the codes (int8 + a scale per row / bf16; IVFPQRefineIPIndex, faiss's IndexRefine); their file is this repository's own
format (faiss_io.py, 'WiPR').  Under a process group the three behave as IndexIVFFlat does: without WISE_SHARDED_IVF=1 rank 0
builds and every rank loads the whole file; with it they are sharded by list-major row ranges (below).

**One process per GPU** (the reference has no distributed path).  When `torch.distributed` is initialised
with more than one rank (or WISE_SHARDED_INDEX=1), the same two calls shard the flat index by rows:
  * `create_index('IndexFlatIP')`: rank r reads ONLY feature-store shard files r, r + W, ... and writes its own part,
    `{media_type}-IndexFlatIP.faiss.part-RRR-of-WWW` (same file layout, ids are the store's global ids) — no collective;
  * `load_index('IndexFlatIP')`: rank r loads its part file if the parts of this world size exist, otherwise rows
    `shard_range(N, r, W)` of the single `.faiss` file — memory-mapped, so a rank touches only its own rows' pages —
    and `self.index` is a `ShardedFlatIPIndex`: `search` / `reconstruct_batch` are then collective (every rank calls
    them with the same arguments and gets the global answer: one all-gather of per-shard top-k + `wise_topk_merge`).
IndexIVFFlat is sharded too when WISE_SHARDED_IVF=1 is also set (opt-in; without it, and without IVF part files, every
rank loads the whole file and rank 0 alone builds it).  The index is then one list-major array cut by `shard_range`
(wise_amd/index/sharded.py: rank r holds the whole centroid table and rows shard_range(N, r, W) of list 0's rows, then
list 1's, ...):
  * `create_index('IndexIVFFlat')`: rank r reads only its own store shard files; the ranks train once on a seeded sample
    of min(N, 100 nlist) rows drawn from all of them (rank 0 trains, the centroids are broadcast), each rank assigns its
    own rows, one all-gather of the per-rank list counts fixes the global order (within a list: by source rank, then
    source order), one all_to_all moves rows and ids to the rank that owns their position, and each rank writes
    `{media_type}-IndexIVFFlat.faiss.part-RRR-of-WWW` — a complete IVF file (all centroids, its clipped lists); the parts
    laid end to end are the single-file layout;
  * `load_index('IndexIVFFlat')`: the rank's part file if the parts of this world size exist, otherwise (with the
    switch on) rows shard_range(N, r, W) of the single file, reading only the lists that overlap them; `self.index` is a
    `ShardedIVFFlatIPIndex`, whose `search` / `reconstruct_batch` are collective and return the one-GPU IVF answer.
`IndexIVFPQ<m>` and `IndexIVFPQ<m>R8` / `R16` take the same two paths under the same switch:
  * `create_index`: the same collective build with a per-row byte payload in place of the fp32 row.  Rank 0 trains the coarse
    stage AND the codebooks on the seeded sample gathered from all ranks; centroids and codebooks are broadcast; each rank
    assigns and encodes its own rows on its GPU (and builds their compact rows and scales); the all_to_all moves codes
    (+ compact rows, scales), ids and positions.  No rank holds fp32 rows other than those of its own store shards.  The part
    files are complete 'IwPQ' / 'WiPR' files with clipped lists;
  * `load_index`: the ranks agree ONCE (an all-reduce of "my part exists") whether all of them read part files or all of them
    read rows shard_range(N, r, W) of the single file, so a missing part cannot mix the two sources; `self.index` is a
    `ShardedIVFPQIPIndex` (one exchange per search) or a `ShardedIVFPQRefineIPIndex` (two: candidates, then re-ranked answers),
    both returning the bits of the one-GPU index over the same centroids, codebooks, codes and stores.
`IndexIVFOPQ<m>` and `IndexIVFOPQ<m>R8` / `R16` are the three IVF+PQ types behind a learned rotation of the residuals (faiss's OPQ;
ivf_pq.py: IVFOPQIPIndex, IVFOPQRefineIPIndex); their file wraps the PQ record in a 'WiOP' record that carries the rotation
(faiss_io.py).  They take every path above as their IndexIVFPQ counterparts do: in the collective build rank 0 also trains the
rotation, which is broadcast with the codebooks; each rank rotates its own rows and, in a search, the query — the rotation is
replicated, so the sharded classes and their exchanges are the same.
`IndexIVFSQ8` is the inverted file over one byte per dimension (faiss's IndexIVFScalarQuantizer, QT_8bit; ivf_sq.py: IVFSQIPIndex;
file: faiss's 'IwSq' record, faiss_io.py).  Under a process group it behaves as the types above: without WISE_SHARDED_IVF=1 rank 0
builds the one file and every rank loads it; with it
  * `create_index`: the same collective build.  Rank 0 trains the coarse stage AND the per-dimension ranges on the seeded sample
    the single-file build draws; the [2d] ranges are broadcast with the centroids; each rank assigns and encodes its own rows on
    its GPU; the payload that travels is the row's d code bytes; each rank writes a complete 'IwSq' part with clipped lists.  The
    parts laid end to end are the codes, ids and offsets of the one-process build, byte for byte;
  * `load_index`: parts or ranges of the single file, decided once for the group as for IndexIVFPQ; `self.index` is a
    `ShardedIVFSQIPIndex` (one exchange per search) that returns the bits of the one-GPU index.
"""
import os
from pathlib import Path

import numpy as np

from ..feature.feature_extractor_factory import FeatureExtractorFactory
from ..feature.store.feature_store_factory import FeatureStoreFactory
from . import faiss_io
from .flat_ip import FlatIPIndex
from .ivf_flat import IVFFlatIPIndex, reference_nlist
from .ivf_pq import (IVFOPQIPIndex, IVFOPQRefineIPIndex, IVFPQIPIndex, IVFPQRefineIPIndex, check_opq_shape, check_pq_shape,
                     check_refine_shape)
from .ivf_sq import IVFSQIPIndex, check_sq_shape
from .mutate import plan_update
from .search_index import SearchIndex
from .selector import SearchParameters, as_selector
from .sharded import (ShardedFlatIPIndex, ShardedIVFFlatIPIndex, ShardedIVFPQIPIndex, ShardedIVFPQRefineIPIndex,
                      ShardedIVFSQIPIndex, shard_range)


def _dist_rank_world():
    """(rank, world, sharded?) of the default process group; (0, 1, False) outside torch.distributed."""
    import torch.distributed as dist

    if dist.is_available() and dist.is_initialized():
        rank, world = dist.get_rank(), dist.get_world_size()
        return rank, world, world > 1 or os.environ.get('WISE_SHARDED_INDEX') == '1'
    return 0, 1, False


def parse_ivfpq_type(index_type, feature_dim=None, family='IndexIVFPQ'):
    """m of 'IndexIVFPQ<m>' ('IndexIVFPQ64' -> 64; the bare name -> d / 4, the finest code the m <= 128 limit allows at
    d = 512), None for any other index type.  With feature_dim the shape is checked (ValueError).  family: the name's stem
    (parse_ivfopq_type reads 'IndexIVFOPQ<m>' through here)."""
    if not index_type.startswith(family):
        return None
    tail = index_type[len(family):]
    if tail and not tail.isdigit():
        return None
    if tail:
        m = int(tail)
    elif feature_dim is None:
        return 0
    else:
        m = feature_dim // 4
        if m > 128:
            raise ValueError(f'{family}: the default m = d / 4 = {m} at d = {feature_dim} exceeds the limit m <= 128; '
                             f'name the code size, {family}<m> (for example {family}{feature_dim // 8})')
    if feature_dim is not None:
        (check_opq_shape if family == 'IndexIVFOPQ' else check_pq_shape)(feature_dim, m)
    return m


def parse_ivfpq_refine_type(index_type, feature_dim=None, family='IndexIVFPQ'):
    """(m, kind) of 'IndexIVFPQ<m>R<kind>' ('IndexIVFPQ64R8' -> (64, 8); m as parse_ivfpq_type reads it, the bare
    'IndexIVFPQR16' included), None for any other index type.  A kind other than 8 or 16 is a ValueError; with feature_dim
    the shapes of the codes and of the store are checked (ValueError)."""
    head, sep, tail = index_type.rpartition('R')
    if not sep or not tail.isdigit() or not tail.isascii():
        return None
    m = parse_ivfpq_type(head, feature_dim, family)
    if m is None:
        return None
    kind = int(tail)
    if kind not in (8, 16):
        raise ValueError(f'{index_type}: the re-ranking stores are R8 (int8 rows and a scale each) and R16 (bf16 rows)')
    if feature_dim is not None:
        check_refine_shape(feature_dim, kind)
    return m, kind


def parse_ivfopq_type(index_type, feature_dim=None):
    """m of 'IndexIVFOPQ<m>' — IndexIVFPQ<m> behind a learned rotation (ivf_pq.py: IVFOPQIPIndex) — read as parse_ivfpq_type reads
    its names (the bare 'IndexIVFOPQ' -> d / 4 under the same m <= 128 rule); None for any other index type."""
    return parse_ivfpq_type(index_type, feature_dim, 'IndexIVFOPQ')


def parse_ivfopq_refine_type(index_type, feature_dim=None):
    """(m, kind) of 'IndexIVFOPQ<m>R<kind>', as parse_ivfpq_refine_type; None for any other index type."""
    return parse_ivfpq_refine_type(index_type, feature_dim, 'IndexIVFOPQ')


def _pq_parsers(index_type):
    """(parse m, parse (m, kind), opq?) for the family index_type belongs to"""
    if index_type.startswith('IndexIVFOPQ'):
        return parse_ivfopq_type, parse_ivfopq_refine_type, True
    return parse_ivfpq_type, parse_ivfpq_refine_type, False


def _sharded_ivf_on():
    return os.environ.get('WISE_SHARDED_IVF') == '1'


def _coll_device():
    """Where the tensors of a collective live: the current GPU on the nccl (RCCL) backend, the host on gloo."""
    import torch
    import torch.distributed as dist

    return torch.device('cuda', torch.cuda.current_device()) if dist.get_backend() == 'nccl' else torch.device('cpu')


class FeatureSearchIndex(SearchIndex):
    # the classes that hold a rank's rows in HBM; CPU tests of the multi-rank wiring put stand-ins here
    flat_index_factory = FlatIPIndex
    ivf_index_factory = IVFFlatIPIndex
    ivfpq_index_factory = IVFPQIPIndex
    ivfpq_refine_index_factory = IVFPQRefineIPIndex
    ivfopq_index_factory = IVFOPQIPIndex
    ivfopq_refine_index_factory = IVFOPQRefineIPIndex
    ivfsq_index_factory = IVFSQIPIndex

    def __init__(self, media_type, asset_id, asset):
        self.media_type = media_type
        self.feature_extractor_id = asset_id

        assert 'features_dir' in asset, "features_dir missing in assets"
        self.features_dir = Path(asset['features_dir'])

        assert 'index_dir' in asset, "index_dir missing in assets"
        self.index_dir = Path(asset['index_dir'])

        self.prompt = {
            'image': 'This is a photo of a ',
            'video': 'This is a photo of a ',
            'audio': 'this is the sound of '
        }

    def get_index_filename(self, index_type):
        return self.index_dir / (self.media_type + '-' + index_type + '.faiss')

    def get_index_part_filename(self, index_type, rank, world):
        """rank's part of a row-sharded flat index built by `world` processes (not in the reference)."""
        fn = self.get_index_filename(index_type)
        return fn.with_name(fn.name + '.part-%03d-of-%03d' % (rank, world))

    def create_index(self, index_type, overwrite=False):
        self.index_dir.mkdir(parents=True, exist_ok=True)
        index_fn = self.get_index_filename(index_type)
        rank, world, sharded = _dist_rank_world()
        parse_m, parse_refine, opq = _pq_parsers(index_type)
        refine = parse_refine(index_type)
        is_pq = parse_m(index_type) is not None or refine is not None
        is_sq = index_type == 'IndexIVFSQ8'
        sharded_ivf = sharded and (index_type == 'IndexIVFFlat' or is_pq or is_sq) and _sharded_ivf_on()
        if sharded and (index_type == 'IndexFlatIP' or sharded_ivf):
            index_fn = self.get_index_part_filename(index_type, rank, world)
        exists = index_fn.exists()
        if sharded_ivf:                             # the build is collective: every rank takes the same decision
            import torch
            import torch.distributed as dist
            flag = torch.tensor([int(exists)], dtype=torch.int64, device=_coll_device())
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)
            exists = bool(flag.item())
        if exists and overwrite is False:
            print(f'{index_type} for {self.media_type} already exists')
            return
        if index_type not in ('IndexFlatIP', 'IndexIVFFlat') and not is_pq and not is_sq:
            raise NotImplementedError(f'{index_type}: IndexFlatIP, IndexIVFFlat and IndexIVFPQ<m> (with its R8 / R16 and '
                                      f'IndexIVFOPQ<m> forms) and IndexIVFSQ8 are the index types WISE builds')
        self.index_type = index_type
        if sharded and (index_type == 'IndexIVFFlat' or is_pq or is_sq) and not sharded_ivf and rank != 0:
            return                                  # k-means needs every row: one rank builds the one file

        feature_store = FeatureStoreFactory.load_store(self.media_type, self.features_dir)
        if sharded and (index_type == 'IndexFlatIP' or sharded_ivf):
            feature_store.enable_read(shard_shuffle=False, shard_slice=(rank, world))   # this rank's shard files only
        else:
            feature_store.enable_read(shard_shuffle=False)
        feature_count = feature_store.feature_count
        feature_dim = feature_store.feature_dim
        if refine is not None:                                                    # a bad shape is refused before any row is read
            pq_m, kind = parse_refine(index_type, feature_dim)
        else:
            pq_m = parse_m(index_type, feature_dim) if is_pq else None
        if is_sq:
            check_sq_shape(feature_dim)

        # the on-disk index is assembled on the host (I/O-bound: tar + unpickle per vector), 512 at a time
        X = np.empty((feature_count, feature_dim), dtype=np.float32)
        ids = np.empty((feature_count,), dtype=np.int64)
        n = 0
        print('Adding feature vectors to index')
        for feature_ids_batch, feature_vectors_batch in feature_store.iter_batch():
            m = len(feature_ids_batch)
            X[n:n + m] = feature_vectors_batch
            ids[n:n + m] = feature_ids_batch
            n += m
        if sharded_ivf:
            self._create_sharded_ivf(X[:n], ids[:n], index_fn, rank, world, index_type=index_type, pq_m=pq_m,
                                     kind=kind if refine is not None else None, opq=opq, sq=is_sq)
            print(f'  saved index part to {index_fn}')
            return
        if index_type == 'IndexIVFFlat' or is_pq or is_sq:
            cell_count = reference_nlist(n)
            train_count = min(n, 100 * cell_count)
            # the reference trains on the first train_count vectors of a shard-shuffled pass (:62-69); a seeded
            # sample of the same size stands in for it
            sample = np.random.default_rng(1234).permutation(n)[:train_count]
            sample.sort()
            print(f'  training {index_type} index with {train_count} features with {cell_count} clusters ...')
            if refine is not None:
                ivf = (IVFOPQRefineIPIndex if opq else IVFPQRefineIPIndex)(feature_dim, cell_count, pq_m, kind)
            elif opq:
                ivf = IVFOPQIPIndex(feature_dim, cell_count, pq_m)
            elif is_sq:
                ivf = IVFSQIPIndex(feature_dim, cell_count)
            else:
                ivf = IVFPQIPIndex(feature_dim, cell_count, pq_m) if is_pq else IVFFlatIPIndex(feature_dim, cell_count)
            ivf.train(X[sample])                    # the coarse stage, then (IndexIVFPQ / SQ8) the codebooks / ranges on its residuals
            for s0 in range(0, n, 1 << 20):
                ivf.add_with_ids(X[s0:s0 + (1 << 20)], ids[s0:s0 + (1 << 20)])
            if opq:
                c, cb, codes, ids_s, off = ivf.lists_host()
                store = {}
                if refine is not None:
                    rows, scales = ivf.store_host()
                    store = dict(kind=kind, k_factor=ivf.k_factor, rows=rows, scales=scales)
                faiss_io.write_ivf_opq_ip(index_fn, ivf.rotation.cpu().numpy(), c, cb, codes, ids_s, off, nprobe=ivf.nprobe, **store)
            elif refine is not None:
                c, cb, codes, ids_s, off = ivf.lists_host()
                rows, scales = ivf.store_host()
                faiss_io.write_ivf_pq_refine_ip(index_fn, c, cb, codes, ids_s, off, kind, ivf.k_factor, rows, scales, nprobe=ivf.nprobe)
            elif is_pq:
                c, cb, codes, ids_s, off = ivf.lists_host()
                faiss_io.write_ivf_pq_ip(index_fn, c, cb, codes, ids_s, off, nprobe=ivf.nprobe)
            elif is_sq:
                c, trained, codes, ids_s, off = ivf.lists_host()
                faiss_io.write_ivf_sq_ip(index_fn, c, trained, codes, ids_s, off, nprobe=ivf.nprobe)
            else:
                c, Xs, ids_s, off = ivf.lists_host()
                faiss_io.write_ivf_flat_ip(index_fn, c, Xs, ids_s, off, nprobe=ivf.nprobe)
        else:
            faiss_io.write_idmap_flat_ip(index_fn, X[:n], ids[:n])
        print(f'  saved index to {index_fn}')

    def _create_sharded_ivf(self, X, ids, part_fn, rank, world, index_type='IndexIVFFlat', pq_m=None, kind=None, opq=False, sq=False):
        """The collective IVF build of create_index (module docstring): X / ids are this rank's store rows.  What travels to the
        rank that owns a row's position is a per-row byte payload: the fp32 row (IndexIVFFlat), or the row's codes followed by its
        compact row and scale (pq_m / kind given: IndexIVFPQ<m>, IndexIVFPQ<m>R<kind>), encoded where the row was read.  opq: the
        IndexIVFOPQ forms of the two — rank 0 also trains the rotation, which is broadcast with the codebooks.  sq: IndexIVFSQ8 —
        rank 0 also trains the [2d] ranges, which are broadcast with the centroids; the payload is the row's d code bytes."""
        import torch
        import torch.distributed as dist

        dev = _coll_device()
        n, d = X.shape
        # global row count and where each rank's rows sit in the concatenation (rank order)
        ns_t = torch.zeros(world, dtype=torch.int64, device=dev)
        dist.all_gather_into_tensor(ns_t, torch.tensor([n], dtype=torch.int64, device=dev))
        ns = ns_t.cpu().numpy()
        src_off = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
        n_total = int(src_off[-1])
        cell_count = reference_nlist(n_total)
        train_count = min(n_total, 100 * cell_count)
        # the single-file build's seeded sample, drawn over the concatenation of every rank's rows
        sample = np.random.default_rng(1234).permutation(n_total)[:train_count]
        sample.sort()
        bounds = np.searchsorted(sample, src_off)
        mine = sample[bounds[rank]:bounds[rank + 1]] - src_off[rank]
        if kind is not None:
            ivf = (self.ivfopq_refine_index_factory if opq else self.ivfpq_refine_index_factory)(d, cell_count, pq_m, kind)
        elif pq_m is not None:
            ivf = (self.ivfopq_index_factory if opq else self.ivfpq_index_factory)(d, cell_count, pq_m)
        elif sq:
            ivf = self.ivfsq_index_factory(d, cell_count)
        else:
            ivf = self.ivf_index_factory(d, cell_count)
        if rank == 0:                               # k-means once, on rank 0; the centroids' bits go to every rank
            parts = [X[mine]]
            for src in range(1, world):
                m = int(bounds[src + 1] - bounds[src])
                if m:
                    buf = torch.empty(m, d, dtype=torch.float32, device=dev)
                    dist.recv(buf, src=src)
                    parts.append(buf.cpu().numpy())
            print(f'  training {index_type} index with {train_count} features with {cell_count} clusters ...')
            ivf.train(np.concatenate(parts))        # the coarse stage, then (IndexIVFPQ / SQ8) the codebooks / ranges on its residuals
            c = ivf.centroids if torch.is_tensor(ivf.centroids) else torch.from_numpy(np.asarray(ivf.centroids))
            c = c.to(dev, torch.float32).contiguous()
        else:
            if len(mine):
                dist.send(torch.from_numpy(np.ascontiguousarray(X[mine])).to(dev), dst=0)
            c = torch.empty(cell_count, d, dtype=torch.float32, device=dev)
        dist.broadcast(c, src=0)
        centroids = c.cpu().numpy()
        ivf.set_centroids(centroids)
        codebooks = None
        if pq_m is not None:                        # the codebooks' bits go to every rank too
            if rank == 0:
                cb = ivf.codebooks if torch.is_tensor(ivf.codebooks) else torch.from_numpy(np.asarray(ivf.codebooks))
                cb = cb.to(dev, torch.float32).contiguous()
            else:
                cb = torch.empty(pq_m, 256, d // pq_m, dtype=torch.float32, device=dev)
            dist.broadcast(cb, src=0)
            codebooks = cb.cpu().numpy()
            ivf.set_codebooks(codebooks)
        rotation = None
        if opq:                                     # ... and the rotation's: every rank rotates its own rows and queries
            if rank == 0:
                rot = ivf.rotation if torch.is_tensor(ivf.rotation) else torch.from_numpy(np.asarray(ivf.rotation))
                rot = rot.to(dev, torch.float32).contiguous()
            else:
                rot = torch.empty(d, d, dtype=torch.float32, device=dev)
            dist.broadcast(rot, src=0)
            rotation = rot.cpu().numpy()
            ivf.set_rotation(rotation)
        trained = None
        if sq:                                      # ... and, IndexIVFSQ8, the ranges': vmin [d], then vdiff [d]
            if rank == 0:
                tr = ivf.trained if torch.is_tensor(ivf.trained) else torch.from_numpy(np.asarray(ivf.trained))
                tr = tr.to(dev, torch.float32).contiguous()
            else:
                tr = torch.empty(2 * d, dtype=torch.float32, device=dev)
            dist.broadcast(tr, src=0)
            trained = tr.cpu().numpy()
            ivf.set_trained(trained[:d], trained[d:])
        # each rank assigns (and encodes) its own rows; the per-rank list counts fix the global list-major order
        if pq_m is None and not sq:
            a = ivf.assign(X)
            fields = [X]
        else:
            a, *fields = ivf.encode_rows(X)         # codes [n,m] u8 (+ compact rows [n,d] i8 / bf16 bits, scales [n] f32); SQ8: [n,d] u8
            a = np.asarray(a, dtype=np.int64)
        # a row's payload: its fields' bytes back to back, padded to whole int32
        widths = [int(np.prod(f.shape[1:], dtype=np.int64)) * f.dtype.itemsize for f in fields]
        w32 = (sum(widths) + 3) // 4
        cnt = torch.from_numpy(np.bincount(a, minlength=cell_count).astype(np.int64)).to(dev)
        allc_t = torch.empty(world, cell_count, dtype=torch.int64, device=dev)
        dist.all_gather_into_tensor(allc_t.view(-1), cnt)
        allc = allc_t.cpu().numpy()
        list_off = np.concatenate([[0], np.cumsum(allc.sum(axis=0))]).astype(np.int64)
        order = np.argsort(a, kind='stable')        # this rank's rows by list, source order within a list
        a_s = a[order]
        first = np.concatenate([[0], np.cumsum(allc[rank])[:-1]]).astype(np.int64)
        gpos = list_off[a_s] + allc[:rank].sum(axis=0)[a_s] + (np.arange(n, dtype=np.int64) - first[a_s])
        # rows, ids and global positions travel as one int32 buffer per row to the rank that owns the position
        his = np.array([shard_range(n_total, r, world)[1] for r in range(world)], dtype=np.int64)
        dest = np.searchsorted(his, gpos, side='right')
        send_counts = np.bincount(dest, minlength=world).astype(np.int64)
        packed = np.zeros((n, w32 + 4), dtype=np.int32)
        pbytes, b0 = packed.view(np.uint8), 0
        for f, w in zip(fields, widths):
            pbytes[:, b0:b0 + w] = np.ascontiguousarray(f[order]).view(np.uint8).reshape(n, w)
            b0 += w
        packed[:, w32:w32 + 2] = ids[order].astype(np.int64).view(np.int32).reshape(n, 2)
        packed[:, w32 + 2:] = gpos.view(np.int32).reshape(n, 2)
        sc = torch.from_numpy(send_counts).to(dev)
        rc = torch.empty(world, dtype=torch.int64, device=dev)
        dist.all_to_all_single(rc, sc)
        recv_counts = rc.cpu().numpy()
        lo, hi = shard_range(n_total, rank, world)
        recv = torch.empty(int(recv_counts.sum()), w32 + 4, dtype=torch.int32, device=dev)
        dist.all_to_all_single(recv, torch.from_numpy(packed).to(dev), output_split_sizes=recv_counts.tolist(),
                               input_split_sizes=send_counts.tolist())
        got = recv.cpu().numpy()
        pos = np.ascontiguousarray(got[:, w32 + 2:]).view(np.int64).reshape(-1) - lo
        if got.shape[0] != hi - lo or not np.array_equal(np.sort(pos), np.arange(hi - lo)):
            raise RuntimeError(f'sharded {index_type} build: rank {rank} received rows that do not tile [{lo}, {hi})')
        ids_loc = np.empty((hi - lo,), dtype=np.int64)
        ids_loc[pos] = np.ascontiguousarray(got[:, w32:w32 + 2]).view(np.int64).reshape(-1)
        gbytes, b0, loc = got.view(np.uint8), 0, []
        for f, w in zip(fields, widths):
            arr = np.empty((hi - lo,) + f.shape[1:], dtype=f.dtype)
            arr[pos] = np.ascontiguousarray(gbytes[:, b0:b0 + w]).view(f.dtype).reshape((got.shape[0],) + f.shape[1:])
            loc.append(arr)
            b0 += w
        off_loc = np.clip(list_off - lo, 0, hi - lo)
        if opq:
            store = {}
            if kind is not None:
                store = dict(kind=kind, k_factor=ivf.k_factor, rows=loc[1] if kind == 8 else loc[1].view(np.uint16),
                             scales=loc[2] if kind == 8 else None)
            faiss_io.write_ivf_opq_ip(part_fn, rotation, centroids, codebooks, loc[0], ids_loc, off_loc, nprobe=ivf.nprobe, **store)
        elif kind is not None:
            rows = loc[1] if kind == 8 else loc[1].view(np.uint16)
            faiss_io.write_ivf_pq_refine_ip(part_fn, centroids, codebooks, loc[0], ids_loc, off_loc, kind, ivf.k_factor, rows,
                                            loc[2] if kind == 8 else None, nprobe=ivf.nprobe)
        elif pq_m is not None:
            faiss_io.write_ivf_pq_ip(part_fn, centroids, codebooks, loc[0], ids_loc, off_loc, nprobe=ivf.nprobe)
        elif sq:
            faiss_io.write_ivf_sq_ip(part_fn, centroids, trained, loc[0], ids_loc, off_loc, nprobe=ivf.nprobe)
        else:
            faiss_io.write_ivf_flat_ip(part_fn, centroids, loc[0], ids_loc, off_loc, nprobe=ivf.nprobe)

    def _sharded_ivf_index(self, f):
        """ShardedIVFFlatIPIndex around a local index holding the slice `f` (a read_ivf_flat_ip(_range) dict)."""
        import torch

        local = self.ivf_index_factory(f["centroids"].shape[1], f["centroids"].shape[0])
        local.set_centroids(f["centroids"])
        local.adopt_lists(torch.from_numpy(f["X"]), torch.from_numpy(f["ids"]), torch.from_numpy(f["list_off"]))
        local.nprobe = f["nprobe"]
        return ShardedIVFFlatIPIndex(local, merge=getattr(local, 'merge_lists', None),
                                     always_exchange=os.environ.get('WISE_SHARDED_INDEX') == '1')

    def _sharded_ivfpq_index(self, f, pos_base):
        """ShardedIVFPQIPIndex / ShardedIVFPQRefineIPIndex around a local index holding the slice `f` (a dict of one of the
        faiss_io PQ readers) that starts at position pos_base of the whole list-major array."""
        import torch

        nlist, d = f["centroids"].shape
        lists = (torch.from_numpy(f["codes"]), torch.from_numpy(f["ids"]), torch.from_numpy(f["list_off"]))
        always = os.environ.get('WISE_SHARDED_INDEX') == '1'
        opq = "rotation" in f                       # a 'WiOP' file: the same wrappers around the rotating local classes
        if "kind" in f:
            factory = self.ivfopq_refine_index_factory if opq else self.ivfpq_refine_index_factory
            local = factory(d, nlist, f["codebooks"].shape[0], f["kind"], k_factor=f["k_factor"])
            rows = torch.from_numpy(f["rows"] if f["kind"] == 8 else f["rows"].view(np.int16))
            lists += (rows, None if f["scales"] is None else torch.from_numpy(f["scales"]))
            wrapper = ShardedIVFPQRefineIPIndex
        else:
            local = (self.ivfopq_index_factory if opq else self.ivfpq_index_factory)(d, nlist, f["codebooks"].shape[0])
            wrapper = ShardedIVFPQIPIndex
        local.set_centroids(f["centroids"])
        local.set_codebooks(f["codebooks"])
        if opq:
            local.set_rotation(f["rotation"])
        local.adopt_lists(*lists, pos_base=int(pos_base))
        local.nprobe = f["nprobe"]
        return wrapper(local, merge=getattr(local, 'merge_lists', None), always_exchange=always)

    def _sharded_ivfsq_index(self, f, pos_base):
        """ShardedIVFSQIPIndex around a local index holding the slice `f` (a read_ivf_sq_ip(_range) dict) that starts at
        position pos_base of the whole list-major array."""
        import torch

        nlist, d = f["centroids"].shape
        local = self.ivfsq_index_factory(d, nlist)
        local.set_centroids(f["centroids"])
        local.set_trained(f["trained"][:d], f["trained"][d:])
        local.adopt_lists(torch.from_numpy(f["codes"]), torch.from_numpy(f["ids"]), torch.from_numpy(f["list_off"]), pos_base=int(pos_base))
        local.nprobe = f["nprobe"]
        return ShardedIVFSQIPIndex(local, merge=getattr(local, 'merge_lists', None),
                                   always_exchange=os.environ.get('WISE_SHARDED_INDEX') == '1')

    def _load_sharded_ivfpq(self, index_fn, part_fn, refine, rank, world, opq=False, sq=False):
        """The sharded load of the IndexIVFPQ family and (sq) of IndexIVFSQ8: all ranks read their part files, or all ranks read
        their range of the single file — decided once for the group."""
        import torch
        import torch.distributed as dist

        dev = _coll_device()
        flag = torch.tensor([int(part_fn.exists())], dtype=torch.int64, device=dev)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        wrap = self._sharded_ivfsq_index if sq else self._sharded_ivfpq_index
        if sq:
            read, read_range, ntotal = faiss_io.read_ivf_sq_ip, faiss_io.read_ivf_sq_ip_range, faiss_io.ivf_sq_ip_ntotal
        elif opq:
            read, read_range, ntotal = faiss_io.read_ivf_opq_ip, faiss_io.read_ivf_opq_ip_range, faiss_io.ivf_opq_ip_ntotal
        elif refine:
            read, read_range, ntotal = faiss_io.read_ivf_pq_refine_ip, faiss_io.read_ivf_pq_refine_ip_range, faiss_io.ivf_pq_refine_ip_ntotal
        else:
            read, read_range, ntotal = faiss_io.read_ivf_pq_ip, faiss_io.read_ivf_pq_ip_range, faiss_io.ivf_pq_ip_ntotal
        if bool(flag.item()):
            f = read(part_fn)
            ns = torch.zeros(world, dtype=torch.int64, device=dev)   # a part starts where the lower ranks' parts end
            dist.all_gather_into_tensor(ns, torch.tensor([f["codes"].shape[0]], dtype=torch.int64, device=dev))
            return wrap(f, int(ns.cpu().numpy()[:rank].sum()))
        if not index_fn.exists():
            have = 'this rank has its part' if part_fn.exists() else 'this rank has no part'
            raise RuntimeError(f'{index_fn}: the part files of {world} ranks are not complete ({have}: {part_fn.name}) and there is '
                               f'no single file to read every rank\'s rows from; parts and a single file are never mixed')
        lo, hi = shard_range(ntotal(index_fn), rank, world)
        return wrap(read_range(index_fn, lo, hi), lo)

    IVF_FOURCCS = ('WiOP', 'WiPR', 'IwPQ', 'IwSq', 'IwFl')

    def _index_from_file(self, fn, shard=None):
        """file -> index object holding the file's rows in HBM, by the file's fourcc; load_index and update_index share it.
        Anything that is not one of IVF_FOURCCS is read as the flat IndexIDMap file (a missing file raises from that reader);
        shard = (rank, world): only rows shard_range(N, rank, world) of a flat file."""
        import torch

        fourcc = faiss_io.index_fourcc(fn) if fn.exists() else None
        if fourcc == 'WiOP':
            f = faiss_io.read_ivf_opq_ip(fn)
            nlist, d = f["centroids"].shape
            lists = (torch.from_numpy(f["codes"]), torch.from_numpy(f["ids"]), torch.from_numpy(f["list_off"]))
            if "kind" in f:
                index = IVFOPQRefineIPIndex(d, nlist, f["codebooks"].shape[0], f["kind"], k_factor=f["k_factor"])
                lists += (torch.from_numpy(f["rows"] if f["kind"] == 8 else f["rows"].view(np.int16)),
                          None if f["scales"] is None else torch.from_numpy(f["scales"]))
            else:
                index = IVFOPQIPIndex(d, nlist, f["codebooks"].shape[0])
            index.set_centroids(f["centroids"])
            index.set_codebooks(f["codebooks"])
            index.set_rotation(f["rotation"])
            index.adopt_lists(*lists)
            index.nprobe = f["nprobe"]
        elif fourcc == 'WiPR':
            f = faiss_io.read_ivf_pq_refine_ip(fn)
            index = IVFPQRefineIPIndex(f["centroids"].shape[1], f["centroids"].shape[0], f["codebooks"].shape[0], f["kind"],
                                       k_factor=f["k_factor"])
            index.set_centroids(f["centroids"])
            index.set_codebooks(f["codebooks"])
            rows = torch.from_numpy(f["rows"] if f["kind"] == 8 else f["rows"].view(np.int16))
            index.adopt_lists(torch.from_numpy(f["codes"]), torch.from_numpy(f["ids"]), torch.from_numpy(f["list_off"]), rows,
                              None if f["scales"] is None else torch.from_numpy(f["scales"]))
            index.nprobe = f["nprobe"]
        elif fourcc == 'IwPQ':
            f = faiss_io.read_ivf_pq_ip(fn)
            index = IVFPQIPIndex(f["centroids"].shape[1], f["centroids"].shape[0], f["codebooks"].shape[0])
            index.set_centroids(f["centroids"])
            index.set_codebooks(f["codebooks"])
            index.adopt_lists(torch.from_numpy(f["codes"]), torch.from_numpy(f["ids"]), torch.from_numpy(f["list_off"]))
            index.nprobe = f["nprobe"]
        elif fourcc == 'IwSq':
            f = faiss_io.read_ivf_sq_ip(fn)
            nlist, d = f["centroids"].shape
            index = IVFSQIPIndex(d, nlist)
            index.set_centroids(f["centroids"])
            index.set_trained(f["trained"][:d], f["trained"][d:])
            index.adopt_lists(torch.from_numpy(f["codes"]), torch.from_numpy(f["ids"]), torch.from_numpy(f["list_off"]))
            index.nprobe = f["nprobe"]
        elif fourcc == 'IwFl':
            f = faiss_io.read_ivf_flat_ip(fn)
            index = IVFFlatIPIndex(f["centroids"].shape[1], f["centroids"].shape[0])
            index.set_centroids(f["centroids"])
            index.adopt_lists(torch.from_numpy(f["X"]), torch.from_numpy(f["ids"]), torch.from_numpy(f["list_off"]))
            index.nprobe = f["nprobe"]
        else:
            X, ids = faiss_io.read_idmap_flat_ip(fn)                 # rows memory-mapped: only [lo, hi) is ever touched
            lo, hi = shard_range(X.shape[0], *shard) if shard is not None else (0, X.shape[0])
            index = self.flat_index_factory(X.shape[1])
            index.reserve(hi - lo)                   # one [n,d] device tensor, filled slice by slice
            for s in range(lo, hi, 1 << 20):         # stream the memory-mapped rows into HBM
                e = min(s + (1 << 20), hi)
                index.add_with_ids(np.ascontiguousarray(X[s:e]), ids[s:e])
        return index

    @staticmethod
    def _write_index_file(index, fn):
        """index object -> file, by the faiss_io writer of its type (the inverse of _index_from_file)."""
        if isinstance(index, FlatIPIndex):
            index._finalize()
            faiss_io.write_idmap_flat_ip(fn, index._X.cpu().numpy(), index._ids.cpu().numpy())
            return
        refine = isinstance(index, IVFPQRefineIPIndex)
        store = {}
        if refine:
            rows, scales = index.store_host()
            store = dict(kind=index.kind, k_factor=index.k_factor, rows=rows, scales=scales)
        if isinstance(index, (IVFOPQIPIndex, IVFOPQRefineIPIndex)):
            c, cb, codes, ids_s, off = index.lists_host()
            faiss_io.write_ivf_opq_ip(fn, index.rotation.cpu().numpy(), c, cb, codes, ids_s, off, nprobe=index.nprobe, **store)
        elif refine:
            c, cb, codes, ids_s, off = index.lists_host()
            faiss_io.write_ivf_pq_refine_ip(fn, c, cb, codes, ids_s, off, store["kind"], store["k_factor"], store["rows"],
                                            store["scales"], nprobe=index.nprobe)
        elif isinstance(index, IVFPQIPIndex):
            c, cb, codes, ids_s, off = index.lists_host()
            faiss_io.write_ivf_pq_ip(fn, c, cb, codes, ids_s, off, nprobe=index.nprobe)
        elif isinstance(index, IVFSQIPIndex):
            c, trained, codes, ids_s, off = index.lists_host()
            faiss_io.write_ivf_sq_ip(fn, c, trained, codes, ids_s, off, nprobe=index.nprobe)
        elif isinstance(index, IVFFlatIPIndex):
            c, Xs, ids_s, off = index.lists_host()
            faiss_io.write_ivf_flat_ip(fn, c, Xs, ids_s, off, nprobe=index.nprobe)
        else:
            raise TypeError(f'{type(index).__name__}: no index file format')

    def update_index(self, index_type):
        """Not in the reference: bring the EXISTING index file of `index_type` in line with the feature store without
        retraining.  The vectors the index holds and the store no longer has are removed (remove_ids: an in-place compaction
        on the GPU); the store's vectors the index lacks are added in store order (add_with_ids: assigned and encoded against
        the centroids, codebooks, rotation and ranges AS TRAINED — nprobe and k_factor stay too); the file is written to a
        temporary name beside it and renamed over it.  Returns (n_added, n_removed); with nothing to do the file is left
        alone.  The feature extractor is not built.  A `self.index` loaded from that file before the call is stale
        afterwards: call load_index again.  Lists are not rebalanced and nothing is retrained, however many updates pile up."""
        parse_m, parse_refine, _ = _pq_parsers(index_type)
        is_pq = parse_m(index_type) is not None or parse_refine(index_type) is not None
        if index_type not in ('IndexFlatIP', 'IndexIVFFlat') and not is_pq and index_type != 'IndexIVFSQ8':
            raise NotImplementedError(f'{index_type}: IndexFlatIP, IndexIVFFlat and IndexIVFPQ<m> (with its R8 / R16 and '
                                      f'IndexIVFOPQ<m> forms) and IndexIVFSQ8 are the index types WISE builds')
        if _dist_rank_world()[2]:
            raise NotImplementedError('update_index under a sharded process group is not built (a collective removal is not): '
                                      'update the single file in one process and shard it again')
        index_fn = self.get_index_filename(index_type)
        if not index_fn.exists():
            raise FileNotFoundError(f'index {index_fn} does not exist; use create_index (the create-index.py script) first')
        index = self._index_from_file(index_fn)
        index_ids = (index._selector_rows()[0]).cpu().numpy()
        feature_store = FeatureStoreFactory.load_store(self.media_type, self.features_dir)
        feature_store.enable_read(shard_shuffle=False)
        if feature_store.feature_dim != index.d:
            raise ValueError(f'update_index: the store holds {feature_store.feature_dim}-d vectors, the index {index.d}-d')
        X = np.empty((feature_store.feature_count, feature_store.feature_dim), dtype=np.float32)
        store_ids = np.empty((feature_store.feature_count,), dtype=np.int64)
        n = 0
        for feature_ids_batch, feature_vectors_batch in feature_store.iter_batch():
            m = len(feature_ids_batch)
            X[n:n + m] = feature_vectors_batch
            store_ids[n:n + m] = feature_ids_batch
            n += m
        remove, add_mask = plan_update(index_ids, store_ids[:n])
        n_removed = index.remove_ids(remove) if remove.size else 0
        add_rows = np.flatnonzero(add_mask)
        for s0 in range(0, add_rows.size, 1 << 20):
            sel = add_rows[s0:s0 + (1 << 20)]
            index.add_with_ids(X[sel], store_ids[sel])
        n_added = int(add_rows.size)
        if n_added or n_removed:
            tmp_fn = index_fn.with_name(index_fn.name + '.tmp-%d' % os.getpid())
            try:
                self._write_index_file(index, tmp_fn)
                os.replace(tmp_fn, index_fn)
            finally:
                if tmp_fn.exists():
                    tmp_fn.unlink()
        print(f'{index_type} for {self.media_type}: added {n_added}, removed {n_removed} vectors')
        return n_added, n_removed

    def is_index_loaded(self):
        return hasattr(self, 'index')

    def load_index(self, index_type):
        index_fn = self.get_index_filename(index_type)
        rank, world, sharded = _dist_rank_world()
        part_fn = self.get_index_part_filename(index_type, rank, world)
        if not index_fn.exists() and not (sharded and part_fn.exists()):
            print(f'  index {index_fn} does not exist')
            print(f'  use create-index.py script to create an index')
        # like the reference (App. B.3) a missing file raises from the reader, it does not return False
        parse_m, parse_refine, opq = _pq_parsers(index_type)
        refine = parse_refine(index_type) is not None
        if sharded and _sharded_ivf_on() and (refine or parse_m(index_type) is not None):
            index = self._load_sharded_ivfpq(index_fn, part_fn, refine, rank, world, opq)
        elif sharded and _sharded_ivf_on() and index_type == 'IndexIVFSQ8':
            index = self._load_sharded_ivfpq(index_fn, part_fn, False, rank, world, sq=True)
        elif sharded and part_fn.exists() and faiss_io.index_fourcc(part_fn) == 'IwFl':
            index = self._sharded_ivf_index(faiss_io.read_ivf_flat_ip(part_fn))      # built by this many ranks
        elif sharded and _sharded_ivf_on() and index_fn.exists() and faiss_io.index_fourcc(index_fn) == 'IwFl':
            lo, hi = shard_range(faiss_io.ivf_flat_ip_ntotal(index_fn), rank, world)
            index = self._sharded_ivf_index(faiss_io.read_ivf_flat_ip_range(index_fn, lo, hi))
        elif index_fn.exists() and faiss_io.index_fourcc(index_fn) in self.IVF_FOURCCS:
            index = self._index_from_file(index_fn)   # unsharded: every rank of a process group loads the whole file
        else:
            if sharded and part_fn.exists():         # built by this many ranks: a rank's part is its shard
                index = self._index_from_file(part_fn)
            else:
                index = self._index_from_file(index_fn, shard=(rank, world) if sharded else None)
            if sharded:
                index = ShardedFlatIPIndex(index, merge=getattr(index, 'merge_lists', None),
                                           always_exchange=os.environ.get('WISE_SHARDED_INDEX') == '1')
        self.index = index
        self.feature_extractor = FeatureExtractorFactory(self.feature_extractor_id)
        return True

    def search(self, media_type, query, topk=5, query_type='text', *, within=None):
        """`within` (not in the reference): an IDSelector (wise_amd/index/selector.py) or an array-like of vector ids — the
        topk best among THOSE vectors, filtered inside the index scan (the reference intersects after the top-k, search.py's
        `in` / `not_in` merges, and so returns fewer than topk).  None: the reference's call, unchanged."""
        if query_type != 'text':
            raise ValueError('query_type={query_type} not implemented')

        if media_type == 'audio':
            if isinstance(query, str):
                media_query_text = [query]
            else:
                media_query_text = [(self.prompt[media_type] + x) for x in query]
        else:
            media_query_text = [(self.prompt[media_type] + query)]

        query_features = self.feature_extractor.extract_text_features(media_query_text)
        if within is None:
            dist, ids = self.index.search(query_features, topk)
        else:
            dist, ids = self.index.search(query_features, topk, params=SearchParameters(sel=as_selector(within)))
        return dist[0], ids[0]

    def search_range(self, media_type, query, threshold, query_type='text', *, within=None):
        """Not in the reference: EVERY vector that scores above `threshold` for the query (faiss's range_search: score > threshold,
        strictly) instead of the topk best — exhaustive retrieval, near-duplicate sweeps, full positive sets.  Same prompt rules
        as `search`; returns (dist, ids) of the first query, by descending score.  On an inverted-file index the hits come from
        the probed lists.  `within`: as on `search`."""
        if query_type != 'text':
            raise ValueError('query_type={query_type} not implemented')

        if media_type == 'audio':
            if isinstance(query, str):
                media_query_text = [query]
            else:
                media_query_text = [(self.prompt[media_type] + x) for x in query]
        else:
            media_query_text = [(self.prompt[media_type] + query)]

        query_features = self.feature_extractor.extract_text_features(media_query_text)
        params = None if within is None else SearchParameters(sel=as_selector(within))
        lims, dist, ids = self.index.range_search(query_features, threshold, params=params)
        return dist[lims[0]:lims[1]], ids[lims[0]:lims[1]]

    def search_batch(self, media_type, queries, topk=5, query_type='text', *, within=None):
        """Not in the reference: what `search` returns for every string of `queries`, from ONE text-tower batch and ONE
        batched index search per 256 of them (wise_amd/search/batch_queries.py; the --queries-from loop of search.py:894-950
        calls `search` row by row).  `within`: as on `search`, one selector for all queries."""
        if query_type != 'text':
            raise ValueError('query_type={query_type} not implemented')
        from ..search.batch_queries import batched_text_search
        return batched_text_search(self, media_type, queries, topk, within=within)
