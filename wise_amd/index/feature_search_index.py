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
and training-sample size chosen as at feature_search_index.py:55-59, k-means and list scan on the GPU).  The other inverted-file
types are the IVF+PQ family of the reference's index study (docs/Search-Index-Evaluation.md:105-123) and its neighbours.  Each is
one entry of FAMILIES below: what it adds to IndexIVFFlat is its trained state, its per-row list payload and its file record.

    index type (example)             class (ivf_flat.py, ivf_pq.py, ivf_sq.py)   trained beyond the centroids   a row in its list             file record (faiss_io.py)
    IndexIVFFlat                     IVFFlatIPIndex          -                              the fp32 row                  'IwFl' (faiss)
    IndexIVFPQ<m> (IndexIVFPQ64)     IVFPQIPIndex            codebooks [m,256,d/m]          m code bytes                  'IwPQ' (faiss)
    IndexIVFPQ<m>R8 / R16            IVFPQRefineIPIndex      codebooks                      codes + a compact row to      'WiPR' (own) around 'IwPQ'
                                                                                            re-rank from: int8 and a
                                                                                            scale (R8) / bf16 (R16)
    IndexIVFOPQ<m>, ...R8 / R16      IVFOPQIPIndex,          codebooks, rotation [d,d]      as their IndexIVFPQ forms     'WiOP' (own) around 'IwPQ'
                                     IVFOPQRefineIPIndex     of the residuals (faiss's OPQ)                               / 'WiPR'
    IndexIVFSQ8                      IVFSQIPIndex            ranges [2d]: vmin, vdiff       d code bytes (QT_8bit)        'IwSq' (faiss)
    IndexIVFSQfp16                   IVFSQfp16IPIndex        -                              d binary16 values (QT_fp16)   'IwSq' (faiss), qtype 4
    IndexIVFFlatL2                   IVFFlatL2Index          - (plain k-means centroids)    the fp32 row; squared-L2      'IwFl' (faiss), metric_type 1,
                                                                                            distances, ascending          'IxF2' quantizer

and the exhaustive types, which have no lists and no training and are the entries of a table of their own (FLAT_TYPES below: the
factory attribute, the shape check, the file's payload, its writer and reader, and the method that takes a file's rows):

    index type                       class (flat_ip.py, flat_sq.py)              a row in HBM and in the file                            file record (faiss_io.py)
    IndexFlatIP                      FlatIPIndex                                 the fp32 row                                            'IxMp' around 'IxFI' (faiss)
    IndexSQfp16                      FlatSQfp16IPIndex                           d binary16 values, 2 d bytes, no fp32 rows              'IxMp' around 'IxSQ' (faiss), qtype 4
    IndexFlatL2 (flat_l2.py)         FlatL2Index                                 the fp32 row; squared-L2 distances, ascending           'IxMp' around 'IxF2' (faiss), metric_type 1
    IndexSQ8bit                      FlatSQ8IPIndex                              d code bytes (QT_8bit) under ranges [2d]: vmin, vdiff   'IxMp' around 'IxSQ' (faiss), qtype 0
    IndexSQfp16L2                    FlatSQfp16L2Index                           d binary16 values; squared-L2 distances, ascending      'IxMp' around 'IxSQ' (faiss), qtype 4, metric_type 1

and the exhaustive product-quantizer types (flat_pq.py), which have no lists but are trained, and so are neither a FAMILIES entry nor a
FLAT_TYPES entry: parse_pq_flat_type reads their names, `^IndexPQ([1-9][0-9]*)(R8|R16)?$` (the code size is always named):

    index type (example)             class (flat_pq.py)                          a row in HBM and in the file                            file record (faiss_io.py)
    IndexPQ<m> (IndexPQ64)           FlatPQIPIndex                               m code bytes under codebooks [m,256,d/m]                'IxMp' around 'IxPq' (faiss)
    IndexPQ<m>R8                     FlatPQRefineIPIndex                         codes + an int8 row and a scale to re-rank from         'WiFR' (own) around 'IxMp' / 'IxPq'
    IndexPQ<m>R16                    FlatPQRefineIPIndex                         codes + a bf16 row to re-rank from                      'WiFR' (own) around 'IxMp' / 'IxPq'

create_index trains their codebooks on the seeded sample of the store an inverted-file build draws (_training_plan: min(N, 100 nlist)
rows), encodes every row on the GPU in chunks of 2^20 and writes codebooks, codes (and compact rows) and ids; load_index hands the
file's codebooks to the index before its codes; update_index adds against the codebooks as trained, and k_factor stays.  Under a process
group they behave as the inverted-file families do WITHOUT WISE_SHARDED_IVF: rank 0 builds the one file and every rank loads the
whole file (row-sharding them is not built).

IndexSQ8bit is the one exhaustive type that carries a trained vector: create_index trains its ranges over EVERY row of the store (a
minimum and a maximum per dimension are exact and order-free, so nothing clamps at build), encodes the rows on the GPU and writes
ranges, codes and ids; load_index hands the file's ranges to the index before its codes; update_index adds against the ranges as
trained (values outside them clamp).  Under a process group the ranks all-reduce their minima and maxima (MIN / MAX) so that every
part holds the one-process build's ranges — a rank whose store slice is empty contributes +max / -max and writes an empty part — and
the skip-if-exists decision is collective for this type (an all-reduce of "my part exists", as for the sharded IVF build).

The classes are one row store and one shared surface (flat_common.py) around their own payload and search.  Wherever IndexFlatIP
is named below — the skip-if-exists build straight from the store, the row-sharded part files, the
ShardedFlatIPIndex wrapper — IndexSQfp16, IndexFlatL2 and IndexSQfp16L2 go the same way (the wrapper exchanges and merges an L2
index's negated distances).  The IndexSQfp16 and IndexSQfp16L2 files differ in the metric_type of their two headers only.  IndexFlatIP and IndexFlatL2 hold the same fp32 payload: the fourcc inside the file's id map tells their files apart,
and an index object's `metric` its type.  The IndexSQfp16 file holds the rows rounded to binary16 (numpy's float32 ->
float16 cast, which is what the GPU encoder of add_with_ids computes bit for bit).

The bare names `IndexIVFPQ` / `IndexIVFOPQ` mean m = d / 4.  Everything below is written once and driven by that table.

**One process** builds an IVF index by training on a seeded sample of min(N, 100 nlist) rows, adding every row, and writing
`index.state_host()` with `faiss_io.write_index`; it loads one with `faiss_io.read_index` and `_local_index`, which rebuilds the
index object from the reader's dict through the family's `*_index_factory` attribute.  `update_index` is that load, `remove_ids` /
`add_with_ids` against the state as trained, and that write.

**One process per GPU** (the reference has no distributed path).  When `torch.distributed` is initialised
with more than one rank (or WISE_SHARDED_INDEX=1), the same two calls shard the flat index by rows:
  * `create_index('IndexFlatIP')`: rank r reads ONLY feature-store shard files r, r + W, ... and writes its own part,
    `{media_type}-IndexFlatIP.faiss.part-RRR-of-WWW` (same file layout, ids are the store's global ids) — no collective;
  * `load_index('IndexFlatIP')`: rank r loads its part file if the parts of this world size exist, otherwise rows
    `shard_range(N, r, W)` of the single `.faiss` file — memory-mapped, so a rank touches only its own rows' pages —
    and `self.index` is a `ShardedFlatIPIndex`: `search` / `reconstruct_batch` are then collective (every rank calls
    them with the same arguments and gets the global answer: one all-gather of per-shard top-k + `wise_topk_merge`).
The inverted-file types are sharded too when WISE_SHARDED_IVF=1 is also set (opt-in; without it, and without part files, rank 0
alone builds the one file — k-means needs every row — and every rank loads all of it).  The index is then one list-major array cut
by `shard_range` (wise_amd/index/sharded.py: rank r holds the whole trained state and rows shard_range(N, r, W) of list 0's rows,
then list 1's, ...):
  * the build (`_create_sharded_ivf`): rank r reads only its own store shard files; rank 0 trains once on the seeded sample the
    one-process build draws, gathered from all ranks; the trained fields are broadcast in the table's order (centroids, codebooks,
    rotation, ranges); each rank assigns and encodes its own rows on its GPU; one all-gather of the per-rank list counts fixes the
    global order (within a list: by source rank, then source order); one all_to_all moves each row's payload bytes, id and
    position to the rank that owns the position — no rank holds fp32 rows other than those of its own store shards, unless they
    are the payload; each rank writes `{media_type}-{index_type}.faiss.part-RRR-of-WWW`, a complete file of its family's record
    with the list sizes clipped to its rows.  The parts laid end to end are the one-process build's file, byte for byte;
  * the load (`_load_sharded_ivf`): the ranks agree ONCE (an all-reduce of "my part exists") whether all of them read part files
    or all of them read rows shard_range(N, r, W) of the single file (`faiss_io.read_index_range` opens only the lists that overlap
    them), so a missing part cannot mix the two sources.  IndexIVFFlat alone keeps an older, rank-local rule (load_index).
    `self.index` is the family's `Sharded*` wrapper around the local index: one exchange per search, two for the R8 / R16 forms
    (candidates, then re-ranked answers), returning the bits of the one-GPU index over the same state.  Rotation, codebooks and
    ranges are replicated, so every rank rotates and encodes its own rows and queries.
"""
import os
import re
from dataclasses import dataclass
from pathlib import Path
from typing import Callable

import numpy as np

from ..feature.feature_extractor_factory import FeatureExtractorFactory
from ..feature.store.feature_store_factory import FeatureStoreFactory
from . import faiss_io
from .flat_ip import FlatIPIndex
from .flat_l2 import FlatL2Index, check_shape as check_flat_l2_shape
from .flat_pq import FlatPQIPIndex, FlatPQRefineIPIndex
from .flat_sq import (FlatSQ8IPIndex, FlatSQfp16IPIndex, FlatSQfp16L2Index, check_shape as check_sqfp16_flat_shape, check_sq8_shape,
                      check_sqfp16_l2_shape)
from .ivf_flat import IVFFlatIPIndex, IVFFlatL2Index, check_l2_shape, reference_nlist
from .ivf_pq import (IVFOPQIPIndex, IVFOPQRefineIPIndex, IVFPQIPIndex, IVFPQRefineIPIndex, check_opq_shape, check_pq_shape,
                     check_refine_shape)
from .ivf_sq import IVFSQfp16IPIndex, IVFSQIPIndex, check_sq_shape
from .mutate import plan_update
from .search_index import SearchIndex
from .selector import IDSelectorGroups, SearchParameters, within_selector
from .sharded import (ShardedFlatIPIndex, ShardedIVFFlatIPIndex, ShardedIVFPQIPIndex, ShardedIVFPQRefineIPIndex,
                      ShardedIVFSQfp16IPIndex, ShardedIVFSQIPIndex, shard_range)


def _always_exchange():
    return os.environ.get('WISE_SHARDED_INDEX') == '1'


def _dist_rank_world():
    """(rank, world, sharded?) of the default process group; (0, 1, False) outside torch.distributed."""
    import torch.distributed as dist

    if dist.is_available() and dist.is_initialized():
        rank, world = dist.get_rank(), dist.get_world_size()
        return rank, world, world > 1 or _always_exchange()
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


_PQ_FLAT_NAME = re.compile(r'^IndexPQ([1-9][0-9]*)(R8|R16)?$')


def parse_pq_flat_type(index_type, feature_dim=None):
    """(m, kind) of 'IndexPQ<m>' / 'IndexPQ<m>R8' / 'IndexPQ<m>R16' ('IndexPQ64' -> (64, None), 'IndexPQ64R8' -> (64, 8)), the
    exhaustive product-quantizer types; None for any other index type — the bare 'IndexPQ', a leading zero and any other suffix among
    them.  With feature_dim the shapes of the codes and of the store are checked (ValueError)."""
    hit = _PQ_FLAT_NAME.fullmatch(index_type)            # (match() would let a trailing newline through at '$')
    if hit is None:
        return None
    m, kind = int(hit.group(1)), (int(hit.group(2)[1:]) if hit.group(2) else None)
    if feature_dim is not None:
        check_pq_shape(feature_dim, m)
        if kind is not None:
            check_refine_shape(feature_dim, kind)
    return m, kind


@dataclass(frozen=True)
class _Family:
    """One inverted-file index family (module docstring)."""
    parse: Callable      # (index_type, feature_dim=None) -> (m, kind) of a name of this family (None where it has none), None for any
    #                      other name; with feature_dim the shapes are checked (ValueError)
    cls: Callable        # () -> the class the one-process build constructs: this module's name for it, looked up at the call
    factory: str         # the FeatureSearchIndex attribute that constructs a rank's index and an index read from a file
    args: Callable       # (d, nlist, m, kind) -> the constructor's arguments
    trained: tuple       # the trained fields beyond the centroids, in broadcast order: (state key = index attribute,
    #                      setter(index, value), shape(d, nlist, m))
    payload: str         # state key of a row's list payload
    wrapper: type        # the Sharded* class around a rank's index
    refine: bool = False  # compact rows beside the codes: 'kind', 'k_factor', 'rows', 'scales' in the state
    extra: tuple = ()    # further (key, value) pairs of the state that are neither trained nor per-row: ('metric', 'l2') tells
    #                      IndexIVFFlatL2's state from IndexIVFFlat's, whose payload key 'X' it shares

    @property
    def marks(self):
        """the state keys that tell this family's reader dict from the others' (faiss_io.write_index picks the record by them)"""
        return ({k for k, _, _ in self.trained} | ({'kind'} if self.refine else set()) | ({self.payload} - {'codes'})
                | {k for k, _ in self.extra})


_CENTROIDS = ('centroids', lambda index, v: index.set_centroids(v), lambda d, nlist, m: (nlist, d))
_CODEBOOKS = ('codebooks', lambda index, v: index.set_codebooks(v), lambda d, nlist, m: (m, 256, d // m))
_ROTATION = ('rotation', lambda index, v: index.set_rotation(v), lambda d, nlist, m: (d, d))
_RANGES = ('trained', lambda index, v: index.set_trained(v[:v.shape[0] // 2], v[v.shape[0] // 2:]), lambda d, nlist, m: (2 * d,))


def _named(name, check=None):
    """the parser of a family of one name and no parameters"""
    def parse(index_type, feature_dim=None):
        if index_type != name:
            return None
        if check is not None and feature_dim is not None:
            check(feature_dim)
        return None, None
    return parse


def _plain(parse_m):
    def parse(index_type, feature_dim=None):
        m = parse_m(index_type, feature_dim)
        return None if m is None else (m, None)
    return parse


_PQ_ARGS, _REFINE_ARGS = (lambda d, nlist, m, kind: (d, nlist, m)), (lambda d, nlist, m, kind: (d, nlist, m, kind))
IVF_FLAT = _Family(_named('IndexIVFFlat'), lambda: IVFFlatIPIndex, 'ivf_index_factory', lambda d, nlist, m, kind: (d, nlist), (), 'X',
                   ShardedIVFFlatIPIndex)
FAMILIES = (
    IVF_FLAT,
    _Family(_plain(parse_ivfpq_type), lambda: IVFPQIPIndex, 'ivfpq_index_factory', _PQ_ARGS, (_CODEBOOKS,), 'codes', ShardedIVFPQIPIndex),
    _Family(parse_ivfpq_refine_type, lambda: IVFPQRefineIPIndex, 'ivfpq_refine_index_factory', _REFINE_ARGS, (_CODEBOOKS,), 'codes',
            ShardedIVFPQRefineIPIndex, refine=True),
    _Family(_plain(parse_ivfopq_type), lambda: IVFOPQIPIndex, 'ivfopq_index_factory', _PQ_ARGS, (_CODEBOOKS, _ROTATION), 'codes',
            ShardedIVFPQIPIndex),
    _Family(parse_ivfopq_refine_type, lambda: IVFOPQRefineIPIndex, 'ivfopq_refine_index_factory', _REFINE_ARGS, (_CODEBOOKS, _ROTATION),
            'codes', ShardedIVFPQRefineIPIndex, refine=True),
    _Family(_named('IndexIVFSQ8', check_sq_shape), lambda: IVFSQIPIndex, 'ivfsq_index_factory', lambda d, nlist, m, kind: (d, nlist),
            (_RANGES,), 'codes', ShardedIVFSQIPIndex),
    _Family(_named('IndexIVFSQfp16', check_sq_shape), lambda: IVFSQfp16IPIndex, 'ivfsqfp16_index_factory',
            lambda d, nlist, m, kind: (d, nlist), (), 'halves', ShardedIVFSQfp16IPIndex),
    _Family(_named('IndexIVFFlatL2', check_l2_shape), lambda: IVFFlatL2Index, 'ivf_l2_index_factory', lambda d, nlist, m, kind: (d, nlist),
            (), 'X', ShardedIVFFlatIPIndex, extra=(('metric', 'l2'),)),
)
_MARKS = set().union(*(fam.marks for fam in FAMILIES))


def _family(index_type):
    """The family index_type names, None for 'IndexFlatIP' and for a name WISE does not build (a re-ranking name with a kind other
    than 8 or 16 is a ValueError)."""
    return next((fam for fam in FAMILIES if fam.parse(index_type) is not None), None)


def _family_of_state(f):
    """The family of a faiss_io reader's dict."""
    return next(fam for fam in FAMILIES if fam.marks == _MARKS & f.keys())


def _host_state(index, fam):
    """index.state_host(), the dict faiss_io.write_index takes.  A stand-in that implements no more than the factory contract of
    the CPU tests has lists_host() alone; its tuple is the family's state in key order."""
    if hasattr(index, 'state_host'):
        return index.state_host()
    keys = ('centroids',) + tuple(k for k, _, _ in fam.trained if k != 'rotation') + (fam.payload, 'ids', 'list_off')
    return dict(zip(keys, index.lists_host()), **dict(fam.extra))


def _unknown_index_type(index_type):
    return NotImplementedError(f'{index_type}: IndexFlatIP, IndexIVFFlat and IndexIVFPQ<m> (with its R8 / R16 and '
                               f'IndexIVFOPQ<m> forms) and IndexIVFSQ8 are the index types WISE builds, and IndexIVFSQfp16, '
                               f'and IndexSQ8bit, and IndexSQfp16, and IndexFlatL2')


def _to_halves(X):
    """[n,d] float16 of float32 rows: numpy's cast — round to nearest even, subnormals kept — the bits wise_sq16_encode gives"""
    with np.errstate(over='ignore'):
        return np.asarray(X, dtype=np.float32).astype(np.float16)


@dataclass(frozen=True)
class _FlatType:
    """One exhaustive index type (module docstring): no training, no lists, row-sharded across ranks."""
    factory: str         # the FeatureSearchIndex attribute that constructs the index a file's rows go to
    check: Callable      # (feature_dim) -> ValueError for a shape the type does not take, before any row is read; None: none
    fourcc: str          # of the index inside the file's id map (faiss_io.index_fourcc(fn, inner=True))
    dtype: type          # of a value of the file's payload, which is the index's own rows_host()[0]
    encode: Callable     # store rows [n,d] float32 -> that payload, on the host
    writer: Callable     # (path, payload, ids) -> the file; a trained type: (path, trained, payload, ids)
    reader: Callable     # path -> (payload [N,d], memory-mapped; ids [N]); a trained type: (trained [2d], payload, ids)
    add: str             # the index method that takes rows of the file's payload and their ids
    metric: str = 'ip'   # the index object's `metric` (flat_common.py): tells the types apart that share a payload dtype
    qtype: int = None    # of the file's ScalarQuantizer record, which tells the 'IxSQ' files apart (faiss_io.flat_sq_qtype)
    trained: bool = False  # the type carries a trained vector [2d] (vmin, vdiff): the index has minmax / set_minmax / set_trained /
    #                        trained_host, the build goes through the index object (encode is unused), and the file holds the vector


FLAT_TYPES = {
    'IndexFlatIP': _FlatType('flat_index_factory', None, 'IxFI', np.float32, lambda X: X, faiss_io.write_idmap_flat_ip,
                             faiss_io.read_idmap_flat_ip, 'add_with_ids'),
    'IndexSQfp16': _FlatType('flat_sqfp16_index_factory', check_sqfp16_flat_shape, 'IxSQ', np.float16, _to_halves,
                             faiss_io.write_idmap_sq16_ip, faiss_io.read_idmap_sq16_ip, 'add_halves_with_ids', qtype=faiss_io.QT_FP16),
    'IndexFlatL2': _FlatType('flat_l2_index_factory', check_flat_l2_shape, 'IxF2', np.float32, lambda X: X, faiss_io.write_idmap_flat_l2,
                             faiss_io.read_idmap_flat_l2, 'add_with_ids', metric='l2'),
    'IndexSQ8bit': _FlatType('flat_sq8_index_factory', check_sq8_shape, 'IxSQ', np.uint8, None, faiss_io.write_idmap_sq8_ip,
                             faiss_io.read_idmap_sq8_ip, 'add_codes_with_ids', qtype=faiss_io.QT_8BIT, trained=True),
    'IndexSQfp16L2': _FlatType('flat_sqfp16_l2_index_factory', check_sqfp16_l2_shape, 'IxSQ', np.float16, _to_halves,
                               faiss_io.write_idmap_sq16_l2, faiss_io.read_idmap_sq16_l2, 'add_halves_with_ids', metric='l2',
                               qtype=faiss_io.QT_FP16),
}


def _sharded_ivf_on():
    return os.environ.get('WISE_SHARDED_IVF') == '1'


def _coll_device():
    """Where the tensors of a collective live: the current GPU on the nccl (RCCL) backend, the host on gloo."""
    import torch
    import torch.distributed as dist

    return torch.device('cuda', torch.cuda.current_device()) if dist.get_backend() == 'nccl' else torch.device('cpu')


def _training_plan(n):
    """(cell count, training rows, their sorted indices) for an IVF index over n rows.  The reference trains on the first
    min(n, 100 nlist) vectors of a shard-shuffled pass (:62-69); a seeded sample of the same size stands in for it."""
    cell_count = reference_nlist(n)
    train_count = min(n, 100 * cell_count)
    sample = np.random.default_rng(1234).permutation(n)[:train_count]
    sample.sort()
    return cell_count, train_count, sample


def _read_store(feature_store):
    """(X [n,d] float32, ids [n]) of every vector the opened store yields, assembled on the host (I/O-bound: tar + unpickle per
    vector), 512 at a time."""
    X = np.empty((feature_store.feature_count, feature_store.feature_dim), dtype=np.float32)
    ids = np.empty((feature_store.feature_count,), dtype=np.int64)
    n = 0
    for feature_ids_batch, feature_vectors_batch in feature_store.iter_batch():
        m = len(feature_ids_batch)
        X[n:n + m] = feature_vectors_batch
        ids[n:n + m] = feature_ids_batch
        n += m
    return X[:n], ids[:n]


class FeatureSearchIndex(SearchIndex):
    # the classes that hold a rank's rows in HBM; CPU tests of the multi-rank wiring put stand-ins here
    flat_index_factory = FlatIPIndex
    flat_sqfp16_index_factory = FlatSQfp16IPIndex
    flat_sqfp16_l2_index_factory = FlatSQfp16L2Index
    flat_l2_index_factory = FlatL2Index
    flat_sq8_index_factory = FlatSQ8IPIndex
    flat_pq_index_factory = FlatPQIPIndex
    flat_pq_refine_index_factory = FlatPQRefineIPIndex
    ivf_index_factory = IVFFlatIPIndex
    ivfpq_index_factory = IVFPQIPIndex
    ivfpq_refine_index_factory = IVFPQRefineIPIndex
    ivfopq_index_factory = IVFOPQIPIndex
    ivfopq_refine_index_factory = IVFOPQRefineIPIndex
    ivfsq_index_factory = IVFSQIPIndex
    ivfsqfp16_index_factory = IVFSQfp16IPIndex
    ivf_l2_index_factory = IVFFlatL2Index

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
        fam = _family(index_type)                   # None: an exhaustive type (or a name refused below)
        flat = FLAT_TYPES.get(index_type)
        pq_flat = parse_pq_flat_type(index_type)    # (m, kind) of an exhaustive product-quantizer type
        sharded_ivf = sharded and fam is not None and _sharded_ivf_on()
        if sharded and (index_type in FLAT_TYPES or sharded_ivf):
            index_fn = self.get_index_part_filename(index_type, rank, world)
        exists = index_fn.exists()
        if sharded_ivf or (sharded and flat is not None and flat.trained):   # the build is collective: every rank takes the same decision
            import torch
            import torch.distributed as dist
            flag = torch.tensor([int(exists)], dtype=torch.int64, device=_coll_device())
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)
            exists = bool(flag.item())
        if exists and overwrite is False:
            print(f'{index_type} for {self.media_type} already exists')
            return
        if index_type not in FLAT_TYPES and fam is None and pq_flat is None:
            raise _unknown_index_type(index_type)
        self.index_type = index_type
        if sharded and ((fam is not None and not sharded_ivf) or pq_flat is not None) and rank != 0:
            return                                  # k-means needs every row: one rank builds the one file

        feature_store = FeatureStoreFactory.load_store(self.media_type, self.features_dir)
        if sharded and (index_type in FLAT_TYPES or sharded_ivf):
            feature_store.enable_read(shard_shuffle=False, shard_slice=(rank, world))   # this rank's shard files only
        else:
            feature_store.enable_read(shard_shuffle=False)
        feature_dim = feature_store.feature_dim
        if fam is not None:                         # a bad shape is refused before any row is read
            pq_m, kind = fam.parse(index_type, feature_dim)
        elif pq_flat is not None:
            parse_pq_flat_type(index_type, feature_dim)
        elif flat.check is not None:
            flat.check(feature_dim)

        print('Adding feature vectors to index')
        X, ids = _read_store(feature_store)
        n = X.shape[0]
        if sharded_ivf:
            self._create_sharded_ivf(X, ids, index_fn, rank, world, index_type, fam, pq_m, kind)
            print(f'  saved index part to {index_fn}')
            return
        if fam is not None:
            cell_count, train_count, sample = _training_plan(n)
            print(f'  training {index_type} index with {train_count} features with {cell_count} clusters ...')
            ivf = fam.cls()(*fam.args(feature_dim, cell_count, pq_m, kind))
            ivf.train(X[sample])                    # the coarse stage, then the family's trained fields on its residuals
            for s0 in range(0, n, 1 << 20):
                ivf.add_with_ids(X[s0:s0 + (1 << 20)], ids[s0:s0 + (1 << 20)])
            faiss_io.write_index(index_fn, _host_state(ivf, fam), nprobe=ivf.nprobe)
        elif pq_flat is not None:
            self._create_pq_flat(X, ids, index_fn, index_type, *pq_flat)
        elif flat.trained:
            self._create_trained_flat(flat, X, ids, index_fn, sharded)
        else:
            flat.writer(index_fn, flat.encode(X), ids)
        print(f'  saved index to {index_fn}')

    def _create_trained_flat(self, flat, X, ids, index_fn, sharded):
        """The build of an exhaustive type with a trained vector (IndexSQ8bit): the ranges over EVERY row — under a process group
        over every rank's rows, one MIN and one MAX all-reduce of the ranks' own minima and maxima; a rank without rows contributes
        +max / -max — then this rank's rows encoded by the index object, and its file.  Collective when sharded."""
        index = getattr(self, flat.factory)(X.shape[1])
        lohi = index.minmax(X)
        if sharded:
            import torch.distributed as dist
            lohi = lohi.to(_coll_device())
            lo, hi = lohi[0].contiguous(), lohi[1].contiguous()
            dist.all_reduce(lo, op=dist.ReduceOp.MIN)
            dist.all_reduce(hi, op=dist.ReduceOp.MAX)
            lohi[0], lohi[1] = lo, hi
        index.set_minmax(lohi)
        index.reserve(X.shape[0])
        for s0 in range(0, X.shape[0], 1 << 20):
            index.add_with_ids(X[s0:s0 + (1 << 20)], ids[s0:s0 + (1 << 20)])
        self._write_index_file(index, index_fn)

    def _new_pq_flat(self, d, m, kind, k_factor=None):
        """The index object of an exhaustive product-quantizer type, from its factory attribute."""
        if kind is None:
            return self.flat_pq_index_factory(d, m)
        return self.flat_pq_refine_index_factory(d, m, kind, **({} if k_factor is None else {'k_factor': k_factor}))

    def _create_pq_flat(self, X, ids, index_fn, index_type, m, kind):
        """The build of IndexPQ<m> and its R8 / R16 forms: the codebooks from the seeded sample an inverted-file build trains on, then
        every row encoded by the index object in chunks of 2^20, and its file."""
        n = X.shape[0]
        _, train_count, sample = _training_plan(n)
        print(f'  training {index_type} index with {train_count} features ...')
        index = self._new_pq_flat(X.shape[1], m, kind)
        index.train(X[sample])
        index.reserve(n)
        for s0 in range(0, n, 1 << 20):
            index.add_with_ids(X[s0:s0 + (1 << 20)], ids[s0:s0 + (1 << 20)])
        self._write_index_file(index, index_fn)

    def _create_sharded_ivf(self, X, ids, part_fn, rank, world, index_type, fam, pq_m=None, kind=None):
        """The collective IVF build of create_index (module docstring): X / ids are this rank's store rows, fam the family of
        index_type, pq_m / kind what its name carries.  What travels to the rank that owns a row's position is a per-row byte
        payload, encoded where the row was read: the fp32 row (IndexIVFFlat), else what the family's encode_rows returns after the
        list — the row's codes, then (re-ranking forms) its compact row and scale."""
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
        # the single-file build's seeded sample, drawn over the concatenation of every rank's rows
        cell_count, train_count, sample = _training_plan(n_total)
        bounds = np.searchsorted(sample, src_off)
        mine = sample[bounds[rank]:bounds[rank + 1]] - src_off[rank]
        ivf = getattr(self, fam.factory)(*fam.args(d, cell_count, pq_m, kind))
        if rank == 0:                               # training once, on rank 0
            parts = [X[mine]]
            for src in range(1, world):
                m = int(bounds[src + 1] - bounds[src])
                if m:
                    buf = torch.empty(m, d, dtype=torch.float32, device=dev)
                    dist.recv(buf, src=src)
                    parts.append(buf.cpu().numpy())
            print(f'  training {index_type} index with {train_count} features with {cell_count} clusters ...')
            ivf.train(np.concatenate(parts))        # the coarse stage, then the family's trained fields on its residuals
        elif len(mine):
            dist.send(torch.from_numpy(np.ascontiguousarray(X[mine])).to(dev), dst=0)
        state = {}
        for key, setter, shape in (_CENTROIDS,) + fam.trained:     # the trained fields' bits go to every rank
            if rank == 0:
                t = getattr(ivf, key)
                t = (t if torch.is_tensor(t) else torch.from_numpy(np.asarray(t))).to(dev, torch.float32).contiguous()
            else:
                t = torch.empty(*shape(d, cell_count, pq_m), dtype=torch.float32, device=dev)
            dist.broadcast(t, src=0)
            state[key] = t.cpu().numpy()
            setter(ivf, state[key])
        # each rank assigns (and encodes) its own rows; the per-rank list counts fix the global list-major order
        if fam.payload == 'X':                      # the fp32 row is the payload (IndexIVFFlat, IndexIVFFlatL2)
            a = ivf.assign(X)
            fields = [X]
        else:
            a, *fields = ivf.encode_rows(X)         # codes [n,m] u8 (+ compact rows [n,d] i8 / bf16 bits, scales [n] f32); SQ8: [n,d] u8; SQfp16: [n,d] f16
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
        state.update({fam.payload: loc[0], 'ids': ids_loc, 'list_off': np.clip(list_off - lo, 0, hi - lo)}, **dict(fam.extra))
        if fam.refine:                              # bf16 rows travel as their bit patterns; the file holds them as uint16
            state.update(kind=kind, k_factor=ivf.k_factor, rows=loc[1] if kind == 8 else loc[1].view(np.uint16),
                         scales=loc[2] if kind == 8 else None)
        faiss_io.write_index(part_fn, state, nprobe=ivf.nprobe)

    def _local_index(self, f, pos_base=None):
        """(family, index object holding the rows of `f` in HBM): f is a dict of faiss_io.read_index / read_index_range, the object
        comes from the family's *_index_factory attribute.  pos_base: where the slice f starts in the whole list-major array (the
        families whose sharded scan reports positions take it)."""
        import torch

        fam = _family_of_state(f)
        nlist, d = f["centroids"].shape
        m = f["codebooks"].shape[0] if "codebooks" in f else None
        index = getattr(self, fam.factory)(*fam.args(d, nlist, m, f.get("kind")), **({"k_factor": f["k_factor"]} if fam.refine else {}))
        for key, setter, _ in (_CENTROIDS,) + fam.trained:
            setter(index, f[key])
        lists = [torch.from_numpy(f[fam.payload]), torch.from_numpy(f["ids"]), torch.from_numpy(f["list_off"])]
        if fam.refine:                              # bf16 rows are uint16 bit patterns in the file, int16 in torch
            lists += [torch.from_numpy(f["rows"] if f["kind"] == 8 else f["rows"].view(np.int16)),
                      None if f["scales"] is None else torch.from_numpy(f["scales"])]
        index.adopt_lists(*lists, **({} if pos_base is None else {"pos_base": int(pos_base)}))
        index.nprobe = f["nprobe"]
        return fam, index

    @staticmethod
    def _sharded(wrapper, local):
        return wrapper(local, merge=getattr(local, 'merge_lists', None), always_exchange=_always_exchange())

    def _sharded_ivf_index(self, f, pos_base=None):
        """The family's Sharded* wrapper around a local index holding the slice `f` (_local_index)."""
        fam, local = self._local_index(f, pos_base)
        return self._sharded(fam.wrapper, local)

    def _load_sharded_ivf(self, index_fn, part_fn, rank, world):
        """The sharded load of every inverted-file family but IndexIVFFlat: all ranks read their part files, or all ranks read
        their range of the single file — decided once for the group."""
        import torch
        import torch.distributed as dist

        dev = _coll_device()
        flag = torch.tensor([int(part_fn.exists())], dtype=torch.int64, device=dev)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        if bool(flag.item()):
            f = faiss_io.read_index(part_fn)
            ns = torch.zeros(world, dtype=torch.int64, device=dev)   # a part starts where the lower ranks' parts end
            dist.all_gather_into_tensor(ns, torch.tensor([f["ids"].shape[0]], dtype=torch.int64, device=dev))
            return self._sharded_ivf_index(f, int(ns.cpu().numpy()[:rank].sum()))
        if not index_fn.exists():
            have = 'this rank has its part' if part_fn.exists() else 'this rank has no part'
            raise RuntimeError(f'{index_fn}: the part files of {world} ranks are not complete ({have}: {part_fn.name}) and there is '
                               f'no single file to read every rank\'s rows from; parts and a single file are never mixed')
        lo, hi = shard_range(faiss_io.index_ntotal(index_fn), rank, world)
        return self._sharded_ivf_index(faiss_io.read_index_range(index_fn, lo, hi), lo)

    IVF_FOURCCS = ('WiOP', 'WiPR', 'IwPQ', 'IwSq', 'IwFl')

    def _index_from_file(self, fn, shard=None):
        """file -> index object holding the file's rows in HBM, by the file's fourcc; load_index and update_index share it.
        An 'IxSQ' file, bare or inside 'IxMp' (the fourcc INSIDE the id map decides, fp32 is not assumed), is an IndexSQfp16 — where its
        record's metric_type is 1, an IndexSQfp16L2 — or, where its ScalarQuantizer record says qtype 0, an IndexSQ8bit, an
        'IxF2' file an IndexFlatL2;
        anything else that is not one of IVF_FOURCCS is read as the flat IndexIDMap file (a missing file raises from that reader);
        shard = (rank, world): only rows shard_range(N, rank, world) of either flat file."""
        if fn.exists() and faiss_io.index_fourcc(fn) in self.IVF_FOURCCS:
            return self._local_index(faiss_io.read_index(fn))[1]
        if self._is_pq_flat_file(fn):
            return self._pq_flat_from_file(fn)
        inner = faiss_io.index_fourcc(fn, inner=True) if fn.exists() else None
        qtype = faiss_io.flat_sq_qtype(fn) if inner == 'IxSQ' else None       # the 'IxSQ' files differ in their record's qtype
        # and the two of qtype 4 in its metric_type (an fp32 file's fourcc names its metric)
        metric = 'l2' if inner == 'IxF2' or (qtype == faiss_io.QT_FP16 and faiss_io.flat_sq_metric(fn) == 1) else 'ip'
        flat = next((t for t in FLAT_TYPES.values() if t.fourcc == inner and t.qtype == qtype and t.metric == metric),
                    FLAT_TYPES['IndexSQfp16' if inner == 'IxSQ' else 'IndexFlatIP'])       # (whose reader refuses the file by name)
        *trained, rows, ids = flat.reader(fn)        # rows memory-mapped: only [lo, hi) is ever touched
        lo, hi = shard_range(rows.shape[0], *shard) if shard is not None else (0, rows.shape[0])
        index = getattr(self, flat.factory)(rows.shape[1])
        if flat.trained:                             # the ranges are whole on every rank
            index.set_trained(trained[0][:rows.shape[1]], trained[0][rows.shape[1]:])
        index.reserve(hi - lo)                       # one [n,d] device tensor, filled slice by slice
        add = getattr(index, flat.add)               # binary16 rows go to HBM as they are: nothing is converted
        for s in range(lo, hi, 1 << 20):             # stream the memory-mapped rows into HBM
            e = min(s + (1 << 20), hi)
            add(np.ascontiguousarray(rows[s:e]), ids[s:e])
        return index

    @staticmethod
    def _is_pq_flat_file(fn):
        """an IndexPQ<m> file ('IxMp' around 'IxPq', or the bare record) or the 'WiFR' file of its R8 / R16 forms"""
        return fn.exists() and (faiss_io.index_fourcc(fn) == 'WiFR' or faiss_io.index_fourcc(fn, inner=True) == 'IxPq')

    def _pq_flat_from_file(self, fn):
        """An IndexPQ<m> / IndexPQ<m>R8 / R16 file -> its index object: the codebooks first, then the memory-mapped codes (and the
        compact rows) streamed into HBM as they are, 2^20 rows at a time."""
        f = faiss_io.read_index(fn)
        m, _, dsub = f['codebooks'].shape
        index = self._new_pq_flat(m * dsub, m, f.get('kind'), f.get('k_factor'))
        index.set_codebooks(f['codebooks'])
        n = f['codes'].shape[0]
        index.reserve(n)
        for s in range(0, n, 1 << 20):
            e = min(s + (1 << 20), n)
            extra = {} if 'kind' not in f else {'rows': f['rows'][s:e], 'scales': None if f['scales'] is None else f['scales'][s:e]}
            index.add_codes_with_ids(np.ascontiguousarray(f['codes'][s:e]), f['ids'][s:e], **extra)
        return index

    @staticmethod
    def _write_index_file(index, fn):
        """index object -> file (the inverse of _index_from_file)."""
        if hasattr(index, 'state_host'):                 # an inverted-file index, or an exhaustive product-quantizer one (no nprobe)
            return faiss_io.write_index(fn, index.state_host(), nprobe=getattr(index, 'nprobe', None))
        payload, ids = index.rows_host()                 # an exhaustive one: its payload's dtype and its metric name the type
        metric = getattr(index, 'metric', 'ip')
        flat = next((t for t in FLAT_TYPES.values() if t.dtype == payload.dtype and t.metric == metric), None)
        if flat is None:
            raise TypeError(f'{type(index).__name__}: no index file format')
        if flat.trained:
            return flat.writer(fn, np.concatenate(index.trained_host()), payload, ids)
        flat.writer(fn, payload, ids)

    def update_index(self, index_type):
        """Not in the reference: bring the EXISTING index file of `index_type` in line with the feature store without
        retraining.  The vectors the index holds and the store no longer has are removed (remove_ids: an in-place compaction
        on the GPU); the store's vectors the index lacks are added in store order (add_with_ids: assigned and encoded against
        the centroids, codebooks, rotation and ranges AS TRAINED — nprobe and k_factor stay too); the file is written to a
        temporary name beside it and renamed over it.  Returns (n_added, n_removed); with nothing to do the file is left
        alone.  The feature extractor is not built.  A `self.index` loaded from that file before the call is stale
        afterwards: call load_index again.  Lists are not rebalanced and nothing is retrained, however many updates pile up."""
        if index_type not in FLAT_TYPES and _family(index_type) is None and parse_pq_flat_type(index_type) is None:
            raise _unknown_index_type(index_type)
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
        X, store_ids = _read_store(feature_store)
        remove, add_mask = plan_update(index_ids, store_ids)
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

    def remove_groups(self, index_type, keys):
        """Not in the reference: "delete these videos" — remove from the EXISTING index file of `index_type` every vector whose
        group key (set_groups: the media id) is in `keys`; the caller passes keys, not vector ids.  Groups are not
        part of an index file, so this NEEDS THE GROUPS SET ON THE LOADED INDEX: load_index(index_type) and set_groups(ids, keys)
        come first (RuntimeError otherwise), and the loaded index must hold the file's vectors (ValueError from set_groups where
        the file holds an id the loaded index has no group for).  Like update_index it works on its own copy of the file — the
        file is loaded, the copy is given the loaded index's groups, its rows go by remove_ids(IDSelectorGroups(keys)), an in-place
        compaction on the GPU, and the file is written to a temporary name beside it and renamed over it — so a `self.index` is
        stale afterwards: call load_index and set_groups again.  COST: because the file holds no groups, every call copies the loaded
        index's ids and per-row keys to the host and builds the copy's group tables there (set_groups: a sort over all N rows) before
        the device-side selector runs — O(N) host work a call, beside reading and writing the file; only the selection of the rows
        is on the device.  Returns the number of vectors removed; with none the file is left
        alone.  The types that take no groups (product-quantized) raise NotImplementedError, as does a sharded process group."""
        if index_type not in FLAT_TYPES and _family(index_type) is None and parse_pq_flat_type(index_type) is None:
            raise _unknown_index_type(index_type)
        if _dist_rank_world()[2]:
            raise NotImplementedError('remove_groups under a sharded process group is not built (a collective removal is not): '
                                      'update the single file in one process and shard it again')
        if not self.is_index_loaded():
            raise RuntimeError('remove_groups: load_index and set_groups first (groups are not part of an index file)')
        index_fn = self.get_index_filename(index_type)
        if not index_fn.exists():
            raise FileNotFoundError(f'index {index_fn} does not exist; use create_index (the create-index.py script) first')
        tables = self.index._need_groups()               # the type's refusal; RuntimeError without groups for the present rows
        row_ids, id_base, n = self.index._selector_rows()
        ids = np.arange(n, dtype=np.int64) + int(id_base) if row_ids is None else row_ids.cpu().numpy()
        keys_of_rows = tables['keys'][tables['gid'].long()].cpu().numpy()
        sel = IDSelectorGroups(keys)                     # non-integer keys are refused before the file is read
        index = self._index_from_file(index_fn)
        index.set_groups(ids, keys_of_rows)
        n_removed = index.remove_ids(sel)
        if n_removed:
            tmp_fn = index_fn.with_name(index_fn.name + '.tmp-%d' % os.getpid())
            try:
                self._write_index_file(index, tmp_fn)
                os.replace(tmp_fn, index_fn)
            finally:
                if tmp_fn.exists():
                    tmp_fn.unlink()
        print(f'{index_type} for {self.media_type}: removed {n_removed} vectors of {np.unique(sel.keys).size} groups')
        return n_removed

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
        fam = _family(index_type)
        if sharded and _sharded_ivf_on() and fam is not None and fam is not IVF_FLAT:
            index = self._load_sharded_ivf(index_fn, part_fn, rank, world)
        # IndexIVFFlat keeps its own, rank-local rule (no all-reduce, and a part file is taken without the switch): the part if it
        # is there, else the rank's range of the single file under WISE_SHARDED_IVF=1.  Only the wrapper's construction is shared.
        elif sharded and part_fn.exists() and faiss_io.index_fourcc(part_fn) == 'IwFl':
            index = self._sharded_ivf_index(faiss_io.read_index(part_fn))             # built by this many ranks
        elif sharded and _sharded_ivf_on() and index_fn.exists() and faiss_io.index_fourcc(index_fn) == 'IwFl':
            lo, hi = shard_range(faiss_io.index_ntotal(index_fn), rank, world)
            index = self._sharded_ivf_index(faiss_io.read_index_range(index_fn, lo, hi))
        elif index_fn.exists() and (faiss_io.index_fourcc(index_fn) in self.IVF_FOURCCS or self._is_pq_flat_file(index_fn)):
            index = self._index_from_file(index_fn)   # unsharded: every rank of a process group loads the whole file
        else:
            if sharded and part_fn.exists():         # built by this many ranks: a rank's part is its shard
                index = self._index_from_file(part_fn)
            else:
                index = self._index_from_file(index_fn, shard=(rank, world) if sharded else None)
            if sharded:
                index = self._sharded(ShardedFlatIPIndex, index)
        self.index = index
        self.feature_extractor = FeatureExtractorFactory(self.feature_extractor_id)
        return True

    def search(self, media_type, query, topk=5, query_type='text', *, within=None, within_groups=None):
        """`within` (not in the reference): an IDSelector (wise_amd/index/selector.py) or an array-like of vector ids — the
        topk best among THOSE vectors, filtered inside the index scan (the reference intersects after the top-k, search.py's
        `in` / `not_in` merges, and so returns fewer than topk).  `within_groups` (not in the reference): an array-like of group
        keys (set_groups: media ids) — the topk best among the vectors of THOSE groups, an IDSelectorGroups resolved on the device
        from the keys alone; with `within` as well, the vectors both select (IDSelectorAnd).  Neither: the reference's call,
        unchanged."""
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
        sel = within_selector(within, within_groups)
        if sel is None:
            dist, ids = self.index.search(query_features, topk)
        else:
            dist, ids = self.index.search(query_features, topk, params=SearchParameters(sel=sel))
        return dist[0], ids[0]

    def search_range(self, media_type, query, threshold, query_type='text', *, within=None, within_groups=None):
        """Not in the reference: EVERY vector that scores above `threshold` for the query (faiss's range_search: score > threshold,
        strictly) instead of the topk best — exhaustive retrieval, near-duplicate sweeps, full positive sets.  Same prompt rules
        as `search`; returns (dist, ids) of the first query, by descending score.  On an inverted-file index the hits come from
        the probed lists.  `within`, `within_groups`: as on `search`."""
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
        sel = within_selector(within, within_groups)
        params = None if sel is None else SearchParameters(sel=sel)
        lims, dist, ids = self.index.range_search(query_features, threshold, params=params)
        return dist[lims[0]:lims[1]], ids[lims[0]:lims[1]]

    def set_groups(self, ids, keys):
        """Not in the reference: keys[i] >= 0 is the group — the media id of a video, a shot, a file — of the vector id ids[i]
        (wise_amd/index/group_search.py).  Every vector of the loaded index needs one; groups are not part of an index file, so
        this follows load_index, and again whatever changes the index's rows."""
        self.index.set_groups(ids, keys)

    def search_grouped(self, media_type, query, topk=5, query_type='text', *, within=None, within_groups=None):
        """Not in the reference, which groups the top `end` rows by media_id after the search (api/routes.py:582-596) and so shows a
        dozen results when the best thousand frames come from a dozen files: the topk best GROUPS, each with its best vector,
        found inside the index scan.  Same prompt rules as `search`; returns (dist, ids, groups) of the first query — the score
        and vector id of each group's best vector and the group's key, best group first.  On an inverted-file index the
        candidates are the vectors of the probed lists.  `within`, `within_groups`: as on `search`; a group none of whose vectors
        is selected does not appear."""
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
        sel = within_selector(within, within_groups)
        params = None if sel is None else SearchParameters(sel=sel)
        dist, ids, groups = self.index.search_grouped(query_features, topk, params=params)
        return dist[0], ids[0], groups[0]

    def search_batch(self, media_type, queries, topk=5, query_type='text', *, within=None, within_groups=None):
        """Not in the reference: what `search` returns for every string of `queries`, from ONE text-tower batch and ONE
        batched index search per 256 of them (wise_amd/search/batch_queries.py; the --queries-from loop of search.py:894-950
        calls `search` row by row).  `within`, `within_groups`: as on `search`, one selector for all queries."""
        if query_type != 'text':
            raise ValueError('query_type={query_type} not implemented')
        from ..search.batch_queries import batched_text_search
        return batched_text_search(self, media_type, queries, topk, within=within_selector(within, within_groups))
