"""Scenes for the dense numerics tests (test_dense_numerics_cpu.py, test_gpu_dense_numerics.py): inputs the unit-norm, positive-score
corpora of the other dense tests never produce.

Every builder is seeded and returns (x16, q16, k, extras); the matching check_* function asserts the scene's PRECONDITIONS from fp64
scores alone (dense_pruning_util: exact_scores, delta_of, bands, comfortable) -- the properties that make a defect visible:

  negative       every score of an "anti" query is < 0: a phantom score of 0 (a row past N, a padding entry, an empty sort slot) outranks
                 every real row
  zeros          80 all-zero rows (+0 and -0) lead the list of an anti query with a score of exactly +0.0; an all-zero query
  subnormal      rows whose ranking is decided by fp16 subnormal elements alone: an instruction that flushes them moves the scores by
                 >= 10 delta and leaves at most 10 of the top 100
  subnormal_q    the same with the roles swapped (the subnormal operand is the query)
  range          row norms spread over >= 2^7, query norm 8; and a twin scaled by exact powers of two
  cancellation   every score within a few delta of zero: the re-score set exceeds its budget, the exhaustive path must answer

No row count is a multiple of 128: the last tile of every tile shape holds rows past N.
"""
import numpy as np

from dense_pruning_util import RESCORE_CAP, bands, comfortable, delta_of, exact_scores, kth_score
from easyrag_amd import synth
from oracle import dense_exact_topk, to_f16_unit

K = 100
F16_TINY = 2.0 ** -14                                                 # smallest normal fp16 magnitude
DIRS_N, DIRS_CLASSES = 9001, (4600, 4401)                             # both >= 4096 (dense_dir_block_min_rows), neither a multiple of 128


def _unit(v):
    return v / np.linalg.norm(v)


def rank_scores(scores, k, mask=None):
    """oracle.dense_exact_topk from a score vector the caller keeps (dense_exact_scores of one query): (score desc, index asc), mask applied,
    first k -- so that masked rankings of one query share one evaluation of the oracle."""
    idx = np.arange(scores.shape[0]) if mask is None else np.flatnonzero(mask)
    s = scores[idx]
    order = np.lexsort((idx, -s))[:k]
    return idx[order].astype(np.int64), s[order]


# ---- negative ---------------------------------------------------------------------------------------------------------------------
def negative_scene(n=8037, d=256, b=600, seed=5):
    """Rows around a unit vector m, "anti" queries around -m (even positions) alternating with ordinary queries (odd positions)."""
    rng = np.random.default_rng(seed)
    m = _unit(rng.standard_normal(d))
    x = to_f16_unit(m + 0.8 * rng.standard_normal((n, d)) / np.sqrt(d))
    q = np.empty((b, d), np.float16)
    anti = np.arange(0, b, 2)
    q[anti] = to_f16_unit(-m + 0.8 * rng.standard_normal((anti.size, d)) / np.sqrt(d))
    q[1::2] = to_f16_unit(synth.dense_queries(x, b - anti.size, seed=seed + 1))
    return x, q, K, {"anti": anti}


def _sampled(q, sample):
    """The queries a check looks at (all of them, or the caller's sample: the large scenes), their fp64 scores come from these rows only."""
    return np.arange(q.shape[0]) if sample is None else np.asarray(sorted(set(int(i) for i in sample)))


def check_negative(x, q, k, extras, sample=None):
    idx = _sampled(q, sample)
    e, dl = exact_scores(x, q[idx]), delta_of(x, q[idx])
    is_anti = np.isin(idx, extras["anti"])
    assert np.count_nonzero(is_anti) >= 2 and np.all(e[is_anti] < 0.0), float(e[is_anti].max())
    assert np.all(e[~is_anti & (idx != extras.get("zero_query", -1))].max(axis=1) > 0.0)   # (the ordinary queries of the batch are ordinary)
    for j in np.flatnonzero(is_anti):
        bd = bands(e[j], kth_score(e[j], k) - 2.0 * dl[j], dl[j], k)
        assert comfortable(bd, k, False), (int(idx[j]), bd)


# ---- zeros ------------------------------------------------------------------------------------------------------------------------
def zeros_scene(n=8037, d=256, b=600, seed=5):
    """The negative scene with 40 all-(+0) rows and 40 all-(-0) rows scattered through it (row 0 and row n - 1 among them) and an
    all-zero query in the last position."""
    x, q, k, extras = negative_scene(n, d, b, seed)
    rng = np.random.default_rng(seed + 100)
    rows = np.sort(np.concatenate([[0, n - 1], rng.choice(np.arange(1, n - 1), size=78, replace=False)]))
    neg = np.zeros(80, bool)
    neg[rng.permutation(np.arange(1, 79))[:39]] = True
    neg[-1] = True                                                    # row 0: +0, row n - 1: -0
    x[rows[~neg]] = np.float16(0.0)
    x[rows[neg]] = np.float16(-0.0)
    q[b - 1] = np.float16(0.0)
    anti = extras["anti"][extras["anti"] != b - 1]
    return x, q, k, {"anti": anti, "zero_rows": rows, "neg_zero_rows": rows[neg], "zero_query": b - 1}


def check_zeros(x, q, k, extras, sample=None, oracle_queries=None):
    zr, zq = extras["zero_rows"], extras["zero_query"]
    assert zr.size == 80 and zr[0] == 0 and zr[-1] == x.shape[0] - 1
    assert np.all(x[zr].view(np.uint16) % 0x8000 == 0)
    assert extras["neg_zero_rows"].size == 40 and np.all(x[extras["neg_zero_rows"]].view(np.uint16) == 0x8000)
    assert np.count_nonzero(np.all(x.view(np.uint16) == 0, axis=1)) == 40
    idx = _sampled(q, sample)
    idx = idx[np.isin(idx, extras["anti"])]
    rest = np.setdiff1d(np.arange(x.shape[0]), zr)
    assert idx.size >= 2 and np.all(exact_scores(x[rest], q[idx]) < 0.0)
    for i in (extras["anti"][:2] if oracle_queries is None else oracle_queries):
        ids, sc = dense_exact_topk(x, q[i], k)
        assert np.array_equal(ids[:80], zr), int(i)
        assert np.all(sc[:80].view(np.uint64) == 0), int(i)           # the bits of +0.0
        assert np.all(sc[80:] < 0.0), int(i)
    ids, sc = dense_exact_topk(x, q[zq], k)
    assert np.array_equal(ids, np.arange(k)) and np.all(sc == 0.0)


# ---- subnormal rows / subnormal queries -------------------------------------------------------------------------------------------
def _subnormal_block(rng, n, d, head_sigma, head=16):
    """n vectors: columns 0..head-1 hold the same normal values in every vector (N(0, head_sigma^2), magnitudes raised to 2^-14 where they
    fall below), the other columns hold +-j * 2^-24, j uniform in [1, 1023] (every one a non-zero fp16 subnormal)."""
    out = np.empty((n, d), np.float16)
    hv = rng.standard_normal(head) * head_sigma
    hv = np.where(hv < 0, -1.0, 1.0) * np.maximum(np.abs(hv), F16_TINY)
    out[:, :head] = hv.astype(np.float16)
    j = rng.integers(1, 1024, size=(n, d - head))
    out[:, head:] = (j * rng.choice([-1.0, 1.0], size=(n, d - head)) * 2.0 ** -24).astype(np.float16)
    return out


def flush_subnormals(a16):
    """What an instruction that flushes fp16 subnormal operands would see."""
    out = a16.copy()
    out[np.abs(out.astype(np.float64)) < F16_TINY] = np.float16(0.0)
    return out


def subnormal_scene(n=6037, d=1024, b=600, seed=3):
    rng = np.random.default_rng(seed)
    x = _subnormal_block(rng, n, d, 0.01)
    q = (2.0 * rng.standard_normal((b, d))).astype(np.float16)
    return x, q, K, {"flushed": "x", "head": 16}


def subnormal_queries_scene(n=6037, d=1024, b=200, seed=4):
    """The roles swapped.  In subnormal_scene the 16 normal columns are equal in every row and cannot rank the rows at all; here the
    normal columns of a query DO rank the rows, so they are four and hold values at the bottom of the normal range (+-2^-14 .. about
    2^-12): the 1020 subnormal columns then decide the ranking (16 columns of N(0, 0.01^2) would leave 95 of the top 100 in place)."""
    rng = np.random.default_rng(seed)
    x = (2.0 * rng.standard_normal((n, d))).astype(np.float16)
    q = _subnormal_block(rng, b, d, 2.0 ** -14, head=4)
    return x, q, K, {"flushed": "q", "head": 4}


def check_subnormal(x, q, k, extras, sample=None, oracle_queries=(0, 1)):
    sub = x if extras["flushed"] == "x" else q
    head = extras["head"]
    tail = sub[:, head:].astype(np.float64)
    assert np.all(tail != 0.0) and np.all(np.abs(tail) < F16_TINY)    # every tail value is a non-zero subnormal
    assert np.all(np.abs(sub[:, :head].astype(np.float64)) >= F16_TINY) and np.all(sub[:, :head] == sub[0, :head])
    idx = _sampled(q, sample)
    oracle_queries = [int(np.flatnonzero(idx == i)[0]) for i in oracle_queries]
    q = q[idx]
    e = exact_scores(x, q)
    ef = exact_scores(flush_subnormals(x), q) if extras["flushed"] == "x" else exact_scores(x, flush_subnormals(q))
    dl = delta_of(x, q)
    moved = np.max(np.abs(e - ef), axis=1) / dl
    assert np.all(moved >= 10.0), float(moved.min())
    for i in range(q.shape[0]):
        bd = bands(e[i], kth_score(e[i], k) - 2.0 * dl[i], dl[i], k)
        assert comfortable(bd, k, False), (i, bd)                     # U <= 2048 and W <= 1024
        top = np.argsort(-e[i], kind="stable")[:k]
        top_f = np.argsort(-ef[i], kind="stable")[:k]
        assert len(set(top.tolist()) & set(top_f.tolist())) <= 10, i
    for i in oracle_queries:                                          # (the oracle itself: 0.3 s per query at d = 1024)
        ids, _ = dense_exact_topk(x, q[i], k)
        top_f = np.argsort(-ef[i], kind="stable")[:k]
        assert len(set(ids.tolist()) & set(top_f.tolist())) <= 10, i


# ---- range ------------------------------------------------------------------------------------------------------------------------
def range_scene(n=8037, d=256, b=200, seed=7):
    """Unit rows times 2^e, e uniform per row in [-3, 5]; unit queries times 8."""
    rng = np.random.default_rng(seed)
    x = (to_f16_unit(rng.standard_normal((n, d))).astype(np.float32) * 2.0 ** rng.integers(-3, 6, size=(n, 1))).astype(np.float16)
    q = (to_f16_unit(rng.standard_normal((b, d))).astype(np.float32) * 8.0).astype(np.float16)
    return x, q, K, {"twin_row_exp": 6, "twin_query_exp": 3}


def range_twin(x, q, extras):
    """Rows x 2^6, queries x 2^3: every score times 2^9."""
    return (np.ldexp(x.astype(np.float32), extras["twin_row_exp"]).astype(np.float16),
            np.ldexp(q.astype(np.float32), extras["twin_query_exp"]).astype(np.float16))


def check_range(x, q, k, extras):
    e = exact_scores(x, q)
    dl = delta_of(x, q)
    norms = np.sqrt(np.sum(x.astype(np.float64) ** 2, axis=1))
    assert norms.max() / norms.min() >= 2.0 ** 7
    for i in range(q.shape[0]):
        bd = bands(e[i], kth_score(e[i], k) - 2.0 * dl[i], dl[i], k)
        assert comfortable(bd, k, False), (i, bd)
    xt, qt = range_twin(x, q, extras)
    assert np.all(np.isfinite(xt)) and np.all(np.isfinite(qt))
    assert np.array_equal(np.ldexp(xt.astype(np.float32), -extras["twin_row_exp"]).astype(np.float16).view(np.uint16), x.view(np.uint16))
    assert np.array_equal(np.ldexp(qt.astype(np.float32), -extras["twin_query_exp"]).astype(np.float16).view(np.uint16), q.view(np.uint16))


# ---- cancellation -----------------------------------------------------------------------------------------------------------------
def cancellation_scene(n=8037, d=256, b=200, seed=9):
    """Row = [u, -u nudged by j ulps] (j in [-2, 2] per element), query = [v, v]: every score is a sum of a few ulps.  (8037 rows: at 6037
    the rows inside kth - 1.9 delta number 1013 for the worst query, fewer than the budget they are to exceed.)"""
    rng = np.random.default_rng(seed)
    h = d // 2
    u = to_f16_unit(rng.standard_normal((n, h)))
    u[u == 0] = np.float16(2.0 ** -10)                                # (a nudge below zero has no meaning)
    w = (-u).view(np.uint16).astype(np.int32) + rng.integers(-2, 3, size=(n, h))   # sign-magnitude: +-1 in the bits is +-1 ulp of |.|
    x = np.concatenate([u, w.astype(np.uint16).view(np.float16)], axis=1)
    v = to_f16_unit(rng.standard_normal((b, h)))
    q = np.concatenate([v, v], axis=1)
    return np.ascontiguousarray(x), np.ascontiguousarray(q), K, {}


def check_cancellation(x, q, k, extras):
    assert np.all(np.isfinite(x))
    e = exact_scores(x, q)
    dl = delta_of(x, q)
    assert np.all(np.max(np.abs(e), axis=1) <= 10.0 * dl)             # within a few delta of zero
    for i in range(q.shape[0]):
        bd = bands(e[i], kth_score(e[i], k) - 2.0 * dl[i], dl[i], k)
        assert bd["W"] > RESCORE_CAP, (i, bd)                         # the final kernel's budget: the exhaustive path must answer
        # (W bounds the device's re-score set from above.  The set itself is {fp32 >= fp32-kth - 2 delta}; these sums of 256 products of
        # ~1e-2 carry an fp32 error of ~1e-4 delta, so it holds every row with E >= kth - 1.9 delta: more than the budget as well)
        assert np.count_nonzero(e[i] >= bd["kth"] - 1.9 * dl[i]) > RESCORE_CAP, (i, bd)


# ---- the same recipes at a size where a batch of 600 queries draws its threshold from the scan kernel's own sample pass ---------------
BIG_N = 80037     # (the pass needs N >= 2 x sampled rows and 4 x rank <= cells: at k = 100 that is N of about 57000 on 256 CUs, 80000 on 128)


BIG_SAMPLE = (0, 1, 2, 255, 256, 511, 598, 599)                       # anti and ordinary queries of every query tile; 599: the zero query


def negative_big_scene(b=600):
    return negative_scene(n=BIG_N, b=b, seed=25)


def zeros_big_scene(b=600):
    return zeros_scene(n=BIG_N, b=b, seed=25)


def subnormal_big_scene(b=600):
    """d = 256: the smallest dimension the persistent scans take (eight K-stages)."""
    return subnormal_scene(n=BIG_N, d=256, b=b, seed=23)


# ---- dirs -------------------------------------------------------------------------------------------------------------------------
def dirs_column(n=DIRS_N, classes=DIRS_CLASSES):
    assert sum(classes) == n and all(c >= 4096 and c % 128 for c in classes) and n % 128
    return np.repeat(np.arange(len(classes)), classes).astype(np.int16)


def negative_dirs_scene(b=64):
    x, q, k, extras = negative_scene(n=DIRS_N, b=b, seed=15)
    return x, q, k, dict(extras, dir_id=dirs_column())


def subnormal_dirs_scene(b=64):
    x, q, k, extras = subnormal_scene(n=DIRS_N, b=b, seed=13)
    return x, q, k, dict(extras, dir_id=dirs_column())


def check_dirs(x, q, k, extras):
    """The scene's own preconditions inside each class (the views the filter produces) and on the whole corpus."""
    e = exact_scores(x, q)
    dl = delta_of(x, q)
    dir_id = extras["dir_id"]
    queries = extras["anti"] if "anti" in extras else np.arange(q.shape[0])
    if "anti" in extras:
        assert np.all(e[queries] < 0.0)
    else:
        ef = exact_scores(flush_subnormals(x), q)
    for c in range(len(DIRS_CLASSES)):
        rows = dir_id == c
        for i in queries:
            ea = e[i][rows]
            bd = bands(ea, kth_score(ea, k) - 2.0 * dl[i], dl[i], k)
            assert comfortable(bd, k, False), (c, int(i), bd)
            if "anti" not in extras:
                assert np.max(np.abs(ea - ef[i][rows])) >= 10.0 * dl[i]
                top, top_f = np.argsort(-ea, kind="stable")[:k], np.argsort(-ef[i][rows], kind="stable")[:k]
                assert len(set(top.tolist()) & set(top_f.tolist())) <= 10, (c, int(i))


# ---- conversions ------------------------------------------------------------------------------------------------------------------
def conversion_matrix(n=300, d=64, seed=21):
    """fp32 values whose rounding to fp16 is delicate: exact halfway points between fp16 neighbours (normal and subnormal range, both
    parities of the lower neighbour), values below 2^-25 (round to zero) and just above it, -0.0, 65504 and 65519 (the largest fp32
    values that still round to a finite fp16 lie below 65520)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)).astype(np.float32)
    flat = x.reshape(-1)
    pos = rng.permutation(flat.size)
    salt = []
    for bits in rng.integers(0x0400, 0x7bff, size=400):              # normal range: halfway between fp16 `bits` and `bits + 1`
        lo, hi = np.array([bits, bits + 1], np.uint16).view(np.float16).astype(np.float64)
        salt.append(0.5 * (lo + hi))
    for j in list(range(0, 64)) + list(rng.integers(64, 1023, size=200)):   # subnormal range: (j + 1/2) * 2^-24 (j = 0: 2^-25 itself)
        salt.append((j + 0.5) * 2.0 ** -24)
    salt += [2.0 ** -26, 2.0 ** -30, 1e-12, 2.0 ** -25 * (1 + 2.0 ** -20), 2.0 ** -24, 2.0 ** -14, 2.0 ** -14 * (1 - 2.0 ** -12)]
    salt += [65504.0, 65519.0, 65519.996, 65503.99]
    salt = np.asarray(salt, np.float64)
    salt = np.concatenate([salt, -salt, [-0.0, 0.0]]).astype(np.float32)
    flat[pos[:salt.size]] = salt
    x[7] = 0.0                                                        # an all-zero row
    return x
