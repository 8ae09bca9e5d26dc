"""numpy restatement of search_grouped (wise_amd/index/group_search.py, csrc/group_topk.hip): given the per-(query, row) scores
of the candidate rows, their positions, the group of every position and the candidate masks, the contract's (D, I, G).

Keys are the scans' (make_key, csrc/topk_common.h): the ordered image of the key score — the score, or the negated distance under
metric 'l2' — above 0xFFFFFFFF - position; 0 stands for "no candidate".  A group's key is the maximum over its candidate rows, the
answer the k largest group keys in descending order, and a key gives back the score's bits, the position and through it the
external id and the group key.  Nothing here shares code with the package.
"""
import numpy as np

PAD = {"ip": np.float32(-3.4028234663852886e38), "l2": np.float32(3.4028234663852886e38)}


def f32_order(s):
    """uint32: the ordered image of float32 values (larger = better), as f32_order of csrc/topk_common.h"""
    u = np.ascontiguousarray(s, dtype=np.float32).view(np.uint32)
    return np.where(u >> np.uint32(31), ~u, u ^ np.uint32(0x80000000)).astype(np.uint32)


def f32_unorder(o):
    o = np.ascontiguousarray(o, dtype=np.uint32)
    u = np.where(o >> np.uint32(31), o ^ np.uint32(0x80000000), ~o).astype(np.uint32)
    return u.view(np.float32)


def make_keys(order, pos):
    """uint64 keys of ordered images `order` (uint32, 0 = no candidate -> key 0) at the positions pos"""
    order = np.asarray(order, dtype=np.uint64)
    low = np.uint64(0xFFFFFFFF) - np.asarray(pos, dtype=np.uint64)
    return np.where(order != 0, (order << np.uint64(32)) | low, np.uint64(0))


def best_keys(ord_, gid, G):
    """[nq, G] uint64 of wise_group_best: per group the maximum key over its rows; ord_ [nq, N] uint32, gid [N] the group of row r"""
    ord_ = np.asarray(ord_, dtype=np.uint32)
    nq, N = ord_.shape
    keys = make_keys(ord_, np.arange(N)[None, :])
    best = np.zeros((nq, G), dtype=np.uint64)
    for q in range(nq):
        np.maximum.at(best[q], np.asarray(gid, dtype=np.int64), keys[q])
    return best


def select(best, k, gid, group_keys, ids=None, id_base=0, metric="ip"):
    """(D [nq,k] float32, I [nq,k] int64, G [nq,k] int64) of wise_group_topk: the k largest keys of every row of best, descending"""
    best = np.asarray(best, dtype=np.uint64)
    nq = best.shape[0]
    D = np.full((nq, k), PAD[metric], dtype=np.float32)
    I = np.full((nq, k), -1, dtype=np.int64)
    Gk = np.full((nq, k), -1, dtype=np.int64)
    for q in range(nq):
        top = np.sort(best[q])[::-1][:k]
        top = top[top != 0]
        pos = (np.uint64(0xFFFFFFFF) - (top & np.uint64(0xFFFFFFFF))).astype(np.int64)
        sc = f32_unorder((top >> np.uint64(32)).astype(np.uint32))
        D[q, :top.size] = -sc if metric == "l2" else sc
        I[q, :top.size] = pos + id_base if ids is None else np.asarray(ids, dtype=np.int64)[pos]
        Gk[q, :top.size] = np.asarray(group_keys, dtype=np.int64)[np.asarray(gid, dtype=np.int64)[pos]]
    return D, I, Gk


def grouped(scores, pos, gid, group_keys, k, mask=None, ids=None, id_base=0, metric="ip"):
    """The contract: scores [nq, M] float32 as the caller sees them (distances under 'l2') of the M rows at the positions pos [M];
    gid [N]: the group of every position; mask [nq, M] or [M] bool: which of them are candidates (None: all)."""
    scores = np.asarray(scores, dtype=np.float32)
    nq, M = scores.shape
    pos = np.asarray(pos, dtype=np.int64)
    order = f32_order(-scores if metric == "l2" else scores)
    if mask is not None:
        order = np.where(np.broadcast_to(np.asarray(mask, dtype=bool), (nq, M)), order, np.uint32(0))
    keys = make_keys(order, pos[None, :])
    G = len(group_keys)
    best = np.zeros((nq, G), dtype=np.uint64)
    g_of = np.asarray(gid, dtype=np.int64)[pos]
    for q in range(nq):
        np.maximum.at(best[q], g_of, keys[q])
    return select(best, k, gid, group_keys, ids, id_base, metric)


def brute_force(scores, pos, gid, group_keys, k, mask=None, ids=None, id_base=0, metric="ip"):
    """The same in plain Python loops over rows (tiny inputs): the contract read literally"""
    nq, M = np.asarray(scores).shape
    out = []
    for q in range(nq):
        rep = {}                                                    # group -> (key score's order, -position) of its representative
        for j in range(M):
            if mask is not None and not np.broadcast_to(np.asarray(mask, dtype=bool), (nq, M))[q, j]:
                continue
            s = np.float32(scores[q][j])
            ks = np.float32(-s) if metric == "l2" else s
            o = int(f32_order(np.array([ks], dtype=np.float32))[0])
            if o == 0:
                continue
            cand = (o, -int(pos[j]), j)
            g = int(gid[int(pos[j])])
            if g not in rep or cand[:2] > rep[g][:2]:
                rep[g] = cand
        ranked = sorted(rep.items(), key=lambda kv: kv[1][:2], reverse=True)[:k]
        row = []
        for g, (_, negp, j) in ranked:
            p = -negp
            row.append((np.float32(scores[q][j]), int(p + id_base if ids is None else ids[p]), int(group_keys[g])))
        row += [(PAD[metric], -1, -1)] * (k - len(row))
        out.append(row)
    D = np.array([[r[0] for r in row] for row in out], dtype=np.float32).reshape(nq, k)
    I = np.array([[r[1] for r in row] for row in out], dtype=np.int64).reshape(nq, k)
    Gk = np.array([[r[2] for r in row] for row in out], dtype=np.int64).reshape(nq, k)
    return D, I, Gk
