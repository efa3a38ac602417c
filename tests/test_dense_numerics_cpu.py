"""The scenes of the dense numerics tests, verified without a GPU: every builder of dense_numerics_util.py with its precondition
function (the properties that make a defect of the kernels visible -- all-negative scores, zero rows in front, rankings decided by
fp16 subnormals, re-score sets beyond the budget), and the scaled-twin identity on the oracle itself."""
import numpy as np
import pytest

import dense_numerics_util as scenes
from oracle import dense_exact_topk
from oracle.dense import dense_exact_scores


@pytest.mark.parametrize("build,check,b", [
    (scenes.negative_scene, scenes.check_negative, 600),
    (scenes.zeros_scene, scenes.check_zeros, 600),
    (scenes.subnormal_scene, scenes.check_subnormal, 600),
    (scenes.subnormal_queries_scene, scenes.check_subnormal, 200),
    (scenes.range_scene, scenes.check_range, 200),
    (scenes.cancellation_scene, scenes.check_cancellation, 200),
    (scenes.negative_dirs_scene, scenes.check_dirs, 64),
    (scenes.subnormal_dirs_scene, scenes.check_dirs, 64),
    (scenes.negative_big_scene, scenes.check_negative, 600),
    (scenes.zeros_big_scene, scenes.check_zeros, 600),
    (scenes.subnormal_big_scene, scenes.check_subnormal, 600),
], ids=["negative", "zeros", "subnormal", "subnormal-queries", "range", "cancellation", "negative-dirs", "subnormal-dirs",
        "negative-80037", "zeros-80037", "subnormal-80037"])
def test_scene_preconditions(build, check, b):
    """At the batch sizes the GPU tests use (the d = 1024 scenes call the oracle itself for two queries, fp64 GEMM scores for all)."""
    x, q, k, extras = build(b=b)
    assert x.dtype == np.float16 and q.dtype == np.float16 and q.shape == (b, x.shape[1]) and k == 100
    assert x.shape[0] % 128 != 0
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(q))
    if x.shape[0] == scenes.BIG_N:
        check(x, q, k, extras, sample=scenes.BIG_SAMPLE)              # (the queries the GPU test holds against the oracle)
    else:
        check(x, q, k, extras)
    x2, q2, _, _ = build(b=b)                                         # seeded: the same bits again
    assert np.array_equal(x.view(np.uint16), x2.view(np.uint16)) and np.array_equal(q.view(np.uint16), q2.view(np.uint16))


def test_scaled_twin_identity_on_the_oracle():
    """Rows x 2^6 and queries x 2^3 scale every product, partial sum and score by 2^9 exactly: same ids, fp64 scores equal bit for bit."""
    x, q, k, extras = scenes.range_scene(b=8)
    xt, qt = scenes.range_twin(x, q, extras)
    for i in range(4):
        ids, sc = dense_exact_topk(x, q[i], k)
        tids, tsc = dense_exact_topk(xt, qt[i], k)
        assert np.array_equal(ids, tids)
        assert np.array_equal(np.ldexp(sc, 9).view(np.uint64), tsc.view(np.uint64))


def test_conversion_matrix_holds_its_salt():
    """The matrix of the conversion test: halfway points in both ranges, values that round to zero, -0.0 and the overflow edge are there,
    and numpy's own conversion (the expectation) keeps everything finite."""
    x = scenes.conversion_matrix()
    assert x.dtype == np.float32 and x.shape == (300, 64)
    h = x.astype(np.float16)
    assert np.all(np.isfinite(h))
    back = h.astype(np.float64)
    x64 = x.astype(np.float64)
    ulp_lo = np.where(np.abs(back) < 2.0 ** -14, 2.0 ** -24, 2.0 ** (np.floor(np.log2(np.maximum(np.abs(back), 2.0 ** -14))) - 10))
    halfway = (np.abs(x64 - back) == 0.5 * ulp_lo) & (x64 != 0)
    assert np.count_nonzero(halfway & (np.abs(x64) >= 2.0 ** -14)) >= 200
    assert np.count_nonzero(halfway & (np.abs(x64) < 2.0 ** -14)) >= 200
    assert np.count_nonzero((x64 != 0) & (np.abs(x64) <= 2.0 ** -25) & (back == 0)) >= 6
    assert np.any(x.view(np.uint32) == 0x80000000) and np.any(x == 65504.0) and np.any(x == 65519.0) and np.any(x == -65519.0)
    assert np.all(x[7] == 0)


def test_rank_scores_is_the_oracle():
    """rank_scores (the GPU tests rank one cached oracle score vector per query under many masks) is oracle.dense_exact_topk, literally:
    ties at +0.0 and an all-tie zero query included, with and without a mask."""
    x, q, k, extras = scenes.zeros_scene(b=8)
    mask = np.arange(x.shape[0]) % 3 != 1
    for i in (0, extras["zero_query"]):
        s = dense_exact_scores(x, q[i])
        for m in (None, mask, np.zeros(x.shape[0], bool)):
            oid, osc = dense_exact_topk(x, q[i], k, m)
            gid, gsc = scenes.rank_scores(s, k, m)
            assert np.array_equal(oid, gid) and np.array_equal(osc.view(np.uint64), gsc.view(np.uint64))
