"""range_search's rules, stated once in numpy (no GPU): what a hit is, how a query's segment is ordered, and the oracle the GPU
tests use — the PREFIX of an existing top-k answer.

  hit       score > float32(thresh), strictly (faiss's rule for METRIC_INNER_PRODUCT): a row whose score equals the threshold
            is not a hit.  The threshold is compared as a float32, the type the kernels take it in.
  order     within a query: descending score — by the scans' sortable key, under which -0.0 sorts below +0.0 —, ties by
            ascending row position (the row of X; the position in list order for the inverted-file types).
  oracle    a top-k answer (D, I) of the same index is ordered the same way, so the hits of a query are exactly its entries
            with D > thresh, a prefix, PROVIDED fewer than k rows are hits; the (-3.4028235e38, -1) padding never is one.
"""
import numpy as np

NEG = np.float32(-3.4028234663852886e38)


def threshold32(thresh) -> np.float32:
    t = np.float32(thresh)
    if not np.isfinite(t):
        raise ValueError(f"thresh={thresh!r} must be finite")
    return t


def f32_order(s):
    """The scans' sortable key of a float32 score (larger = better)."""
    u = np.ascontiguousarray(s, dtype=np.float32).view(np.uint32)
    return np.where(u >> np.uint32(31), ~u, u | np.uint32(0x80000000)).astype(np.int64)


def is_hit(scores, thresh):
    return np.asarray(scores, dtype=np.float32) > threshold32(thresh)


def prefix(D, I, thresh):
    """(D[:n], I[:n]) of one query's top-k answer: its entries that are hits.  The answer must be in the contract's order and the
    hits must form a prefix that ends before k (otherwise the top-k answer was too short to be an oracle)."""
    D, I = np.asarray(D, dtype=np.float32), np.asarray(I, dtype=np.int64)
    hit = is_hit(D, thresh) & (I != -1)
    n = int(hit.sum())
    assert hit[:n].all(), "the hits of a top-k answer are a prefix"
    assert n < len(D), "the top-k answer is full of hits: it cannot show where they end"
    assert (np.diff(f32_order(D[:n])) <= 0).all()
    return D[:n].copy(), I[:n].copy()


def order(scores, positions):
    """The permutation that puts one query's hits into the contract's order."""
    return np.lexsort((np.asarray(positions, dtype=np.int64), -f32_order(scores)))


def in_order(scores, positions) -> bool:
    return np.array_equal(order(scores, positions), np.arange(len(scores)))
