"""The corpus-sharded merge stated in numpy -- the yardstick of tests/test_corpus_shards_cpu.py (where it is held against
hand cases) and of the kernel tests in tests/test_gpu_corpus_shards.py.

A rank's list for one query is (ids int32[k], scores float64[k], len); the global list is: concatenate the live entries with
the rank's first row added to the ids, order by (score descending, global id ascending), cut at k.  The dual route merges
both routes this way and hands them to the oracle's reciprocal_rank_fusion as [sparse, dense]."""
import numpy as np

from oracle import reciprocal_rank_fusion
from oracle.retrievers import Item


def row_bytes(k):
    return (12 * k + 4 + 7) // 8 * 8


def merge_one(ids, sc, ln, id_base, k):
    """ids / sc: [world][k] (one query), ln: [world] -> (global ids int64[<= k], scores float64[<= k])."""
    g = np.concatenate([np.asarray(ids[r][:ln[r]], np.int64) + int(id_base[r]) for r in range(len(ln))])
    s = np.concatenate([np.asarray(sc[r][:ln[r]], np.float64) for r in range(len(ln))])
    order = np.lexsort((g, -s))[:k]
    return g[order], s[order]


def merge_batch(ids, sc, ln, id_base, k):
    """ids / sc: [world, B, k], ln: [world, B] -> padded (ids int32[B, k], scores float64[B, k], len int32[B])."""
    world, B = ln.shape
    o_ids = np.full((B, k), -1, np.int32)
    o_sc = np.zeros((B, k), np.float64)
    o_ln = np.zeros(B, np.int32)
    for q in range(B):
        g, s = merge_one(ids[:, q], sc[:, q], ln[:, q], id_base, k)
        o_ln[q] = g.size
        o_ids[q, :g.size] = g
        o_sc[q, :g.size] = s
    return o_ids, o_sc, o_ln


def merge_rrf_one(sp, dn, id_base, k_sparse, k_dense, content_id, K, topk):
    """sp / dn: (ids [world][k], sc [world][k], ln [world]) of one query -> [(global id, fused score)] of the dual route."""
    gs, ss = merge_one(*sp, id_base, k_sparse)
    gd, sd = merge_one(*dn, id_base, k_dense)
    A = [Item(int(i), int(content_id[i]), float(s)) for i, s in zip(gs, ss)]
    Bl = [Item(int(i), int(content_id[i]), float(s)) for i, s in zip(gd, sd)]
    return [(w.idx, w.score) for w in reciprocal_rank_fusion([A, Bl], K=K, topk=topk)]


def pack_rows(ids, sc, ln):
    """[world, B, k] lists -> what an all-gather of erh_pack_topk rows delivers: uint8 [world, B, row_bytes(k)]."""
    world, B, k = ids.shape
    out = np.zeros((world, B, row_bytes(k)), np.uint8)
    out[:, :, :8 * k] = np.ascontiguousarray(sc, np.float64).view(np.uint8).reshape(world, B, 8 * k)
    out[:, :, 8 * k:12 * k] = np.ascontiguousarray(ids, np.int32).view(np.uint8).reshape(world, B, 4 * k)
    out[:, :, 12 * k:12 * k + 4] = np.ascontiguousarray(ln, np.int32).reshape(world, B, 1).view(np.uint8)
    return out


def random_lists(rng, world, B, k, slice_rows, tie_levels=0, empty_rank=None):
    """Canonical per-rank lists over slices of `slice_rows` rows each: ragged lengths, local ids without repeats; tie_levels > 0
    draws the scores from that many float64 values, so that equal bits meet across ranks and inside a list."""
    ids = np.full((world, B, k), -1, np.int32)
    sc = np.zeros((world, B, k), np.float64)
    ln = np.zeros((world, B), np.int32)
    levels = rng.random(max(tie_levels, 1)) + 0.5
    for r in range(world):
        for q in range(B):
            n = int(rng.integers(0, min(k, slice_rows) + 1))
            if q % 7 == 0:
                n = min(k, slice_rows)                           # full lists as well
            if empty_rank is not None and r == empty_rank:
                n = 0
            loc = rng.choice(slice_rows, size=n, replace=False).astype(np.int64)
            s = levels[rng.integers(0, tie_levels, size=n)] if tie_levels else rng.standard_normal(n)
            order = np.lexsort((loc, -s))
            ids[r, q, :n], sc[r, q, :n], ln[r, q] = loc[order], s[order], n
    return ids, sc, ln
