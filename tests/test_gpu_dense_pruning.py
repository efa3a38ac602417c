"""GPU, dense route: the PRUNING is tested, not only the answers.

Every stage of the pruned pipeline has a safety net: a query whose candidate list, gather or re-score set overflows, or whose speculative
threshold does not verify, is flagged and answered by the exhaustive path (a flagged group of a grouped launch is run again).  A defect in a
threshold, an epilogue or the verification that only flags MORE queries therefore passes every id / score comparison bit for bit.  These
tests read the per-query pruning state (erh_debug_dense_query_state: threshold, candidate count, reason bits) and hold it against counts
derived from plain fp64 scores (tests/dense_pruning_util.py):

  (a) the scan's candidate count lies in [L, U], a band ~2 delta wide that holds a handful of rows;
  (b) a flag must be justified: a comfortable query is never flagged, a speculation that cannot verify is always caught (bit 8), the
      constructed overflows carry their reason bit, and dense_exhaustive_queries counts exactly the flagged queries;
  (c) a threshold that is a guaranteed bound is not "verified" (grouped launch, single block group, unrouted): no flag, no re-run;
  (d) ERH_DENSE_FAST is a ranking: nothing clearly above the exact k-th score is missing, nothing clearly below it is listed, no id
      twice, scores within 1.01 delta of the exact ones (not 1e-3), order right up to 2 delta.
"""
import numpy as np
import pytest

from dense_pruning_util import (FLAG_GATHER, FLAG_LIST, FLAG_SPECULATION, GATHER_CAP, LIST_CAP, bands, check_fast_ranking, comfortable,
                                delta_of, exact_scores, kth_score, speculative)
from easyrag_amd import _lib, synth
from oracle import dense_exact_topk, to_f16_unit

pytestmark = pytest.mark.gpu

# n, d, queries, k, n0: the smallest shapes that reach each mechanism (d = 64: below the persistent scan's eight K-stages; 256; 1024;
# the reference's 3584 with the final kernel's d > 2048 tail; 40000 rows with a deep k)
SHAPES = [(6000, 64, 64, 10, 1024), (12000, 256, 64, 100, 2048), (20000, 1024, 32, 288, 4096), (8000, 3584, 8, 100, 2048),
          (40000, 256, 64, 288, 4096)]
SWEEP = SHAPES[1]                                                     # the 256-d shape carries the batch-size sweep
SWEEP_B = (1, 16, 17, 64, 65, 128, 129, 256, 257)
B_MAX = {(12000, 256): 257, (40000, 256): 512}                        # (the sweep's largest batch, the sample pass' 512 queries)
_DATA = {}


def _data(n, d, b):
    """Corpus, fp16 unit queries, E and delta of a shape: a pure function of (n, d) -- computed once, shared, never written to."""
    key = (n, d)
    if key not in _DATA:
        x = synth.dense_corpus(n, d, seed=n + d)
        q16 = to_f16_unit(synth.dense_queries(x, max(b, B_MAX.get(key, 0)), seed=n + d + 1))
        e = exact_scores(x, q16)
        dl = delta_of(x, q16)
        for a in (x, q16, e, dl):
            a.setflags(write=False)
        _DATA[key] = (x, q16, e, dl)
    x, q16, e, dl = _DATA[key]
    return x, q16[:b], e[:b], dl[:b]


def _seed_rank(k, n0, n):
    return int(_lib.load().erh_dense_seed_rank(int(k), int(n0), int(n)))


def _check_call(engine, x, q16, e, dl, k, speculative, allowed=None, want_comfortable=True, what=""):
    """One EXACT call + one FAST call on (x, q16) with the engine's current options; (a), (b) and (d) for EVERY query of the batch.
    speculative: bool, or one per query; allowed: None, or a boolean mask of A(q) per query (None entries: all rows)."""
    b = q16.shape[0]
    filt = None if allowed is None else allowed[0]
    masks = [None] * b if allowed is None else allowed[1]
    spec = np.broadcast_to(np.asarray(speculative, bool), (b,))
    engine.reset_stats()
    ids, sc, ln = engine.dense_topk(q16, k, filter_dir=filt, mode=_lib.ERH_DENSE_EXACT)
    tau, cnt, flag = engine.dense_query_state(b)
    exhaustive = engine.stat("dense_exhaustive_queries")
    diag = engine.dense_diag()
    fids, fsc, fln = engine.dense_topk(q16, k, filter_dir=filt, mode=_lib.ERH_DENSE_FAST)
    assert diag["uncertified"] == 0 and diag["max_abs_err"] <= diag["margin"], diag
    n_comfortable = 0
    for i in range(b):
        ea = e[i] if masks[i] is None else e[i][masks[i]]
        bd = bands(ea, tau[i], dl[i], k)
        tag = f"{what} query {i}: tau {tau[i]!r} cand_cnt {cnt[i]} flag {flag[i]} {bd}"
        assert np.isfinite(tau[i]) or tau[i] == -np.inf, tag
        # (a) every allowed row with fp32 >= tau is recorded exactly once: E >= tau + dh surely is, E < tau - dh surely is not
        if cnt[i] <= LIST_CAP:
            assert bd["L"] <= cnt[i] <= bd["U"], tag
        # (b) flags must be justified
        ok = comfortable(bd, k, bool(spec[i]))
        n_comfortable += ok
        if ok:
            assert flag[i] == 0, tag
        if spec[i] and bd["verifiable"] and bd["n_lo"] < k:
            assert flag[i] & FLAG_SPECULATION, tag
        # the exact list agrees with the fp64 scores it was checked against elsewhere bit for bit: same rows up to ties at 1e-15
        kk = min(k, ea.shape[0])
        assert ln[i] == kk and fln[i] == kk, tag
        if kk:
            assert abs(sc[i, kk - 1] - bd["kth"]) <= 1e-12 and np.max(np.abs(sc[i, :kk] - e[i][ids[i, :kk]])) <= 1e-12, tag
        # (d) FAST mode as a ranking
        check_fast_ranking(fids[i, :fln[i]], fsc[i, :fln[i]], e[i], masks[i], k, bd["dh"], what=f"{what} query {i} (FAST)")
    assert exhaustive == int(np.count_nonzero(flag)), (what, exhaustive, flag)
    assert diag["exhaustive"] == exhaustive, (what, diag, exhaustive)
    if want_comfortable:                                              # a badly chosen case fails; it cannot pass vacuously
        assert 10 * n_comfortable >= 9 * b, f"{what}: only {n_comfortable} of {b} queries are comfortable"
    return tau, cnt, flag


@pytest.fixture
def dense_opts(engine):
    """Options the cases of this file move, put back whatever happens."""
    yield engine
    for name, value in (("dense_n0", 32768), ("dense_n1", 131072), ("dense_gemv", 1), ("dense_shuffle", 1), ("dense_selfseed", 1),
                        ("dense_dir_blocks", 1), ("dense_dir_block_min_rows", 4096), ("dense_group_sample", 1), ("dense_group_launch", 1),
                        ("n_cus", 0)):
        engine.set_option(name, value)


@pytest.mark.parametrize("gemv", [0, 1], ids=["store-kernel-seed-padded-scan", "skinny-gemm-stream"])
@pytest.mark.parametrize("n,d,b,k,n0", SHAPES)
def test_scan_bookkeeping_and_flags(dense_opts, n, d, b, k, n0, gemv):
    """The default single-stage scheme: store kernel + seed select (speculative rank where it falls below k) + ONE scan of the rest, on the
    padded 256-query scan (half a query tile at <= 128 queries) and on the skinny-GEMM stream of batches up to 64."""
    engine = dense_opts
    x, q16, e, dl = _data(n, d, b)
    engine.set_option("dense_n0", n0)
    engine.set_option("dense_gemv", gemv)
    engine.set_dense(x)
    _check_call(engine, x, q16, e, dl, k, speculative(k, n0, n), what=f"{(n, d, b, k, n0)} gemv={gemv}")
    assert engine.stat("dense_scan_gemv_launches") == 2 * gemv        # the arm under test answered (the EXACT and the FAST call)


@pytest.mark.parametrize("b,gemv", [(b, 0) for b in SWEEP_B] + [(b, 1) for b in SWEEP_B if b <= 64],
                         ids=[f"{b}-padded-scan" for b in SWEEP_B] + [f"{b}-skinny-gemm-stream" for b in SWEEP_B if b <= 64])
def test_scan_bookkeeping_batch_sizes(dense_opts, b, gemv):
    """Batch sizes around every switch of the scan: one query, one / two / four column groups of the skinny-GEMM stream (batches of at
    most 64), half and whole query tiles, a second query tile with one row."""
    engine = dense_opts
    n, d, _, k, n0 = SWEEP
    x, q16, e, dl = _data(n, d, max(SWEEP_B))
    engine.set_option("dense_n0", n0)
    engine.set_option("dense_gemv", gemv)
    engine.set_dense(x)
    _check_call(engine, x, q16[:b], e[:b], dl[:b], k, speculative(k, n0, n), what=f"B={b} gemv={gemv}")


@pytest.mark.parametrize("n,d,b,k,n0", SHAPES[:2])
def test_scan_bookkeeping_whole_view_inside_the_prefix(dense_opts, n, d, b, k, n0):
    """N <= n0: the store kernel scores everything, the threshold is the k-th best of the whole view (a guaranteed bound), no scan stage."""
    engine = dense_opts
    x, q16, e, dl = _data(n, d, b)
    engine.set_option("dense_n0", 32768)
    engine.set_option("dense_gemv", 0)
    engine.set_dense(x)
    tau, cnt, flag = _check_call(engine, x, q16, e, dl, k, False, what=f"{(n, d, b, k)} inside the prefix")
    assert not np.any(flag)
    # a whole-view threshold: the fp32 k-th lies within delta of the exact one, so tau = fp32-kth - 2 delta is pinned by the oracle alone
    for i in range(b):
        kth = kth_score(e[i], k)
        assert kth - 3.03 * dl[i] <= tau[i] <= kth - 0.97 * dl[i], (i, tau[i], kth, dl[i])


def test_scan_bookkeeping_filter_column(dense_opts):
    """The filter column (dense_dir_blocks = 0): A(q) is the query's dir, for the seed select and for the scan's epilogue alike."""
    engine = dense_opts
    n, d, b, k, n0 = SWEEP
    x, q16, e, dl = _data(n, d, max(SWEEP_B))
    q16, e, dl = q16[:b], e[:b], dl[:b]
    dir_id = (np.arange(n) % 3).astype(np.int16)
    filt = (np.arange(b) % 4 - 1).astype(np.int16)                    # -1 (no filter), 0, 1, 2
    masks = [None if f < 0 else dir_id == f for f in filt]
    engine.set_option("dense_n0", n0)
    engine.set_option("dense_dir_blocks", 0)
    engine.set_dense(x)
    engine.set_doc_meta(n, None, dir_id)
    try:
        for gemv in (0, 1):
            engine.set_option("dense_gemv", gemv)
            _check_call(engine, x, q16, e, dl, k, speculative(k, n0, n), allowed=(filt, masks), what=f"filter column gemv={gemv}")
    finally:
        engine.set_doc_meta(n, None, None)


def test_scan_bookkeeping_sample_pass(dense_opts):
    """512 queries on 40000 rows: the scan kernel draws its own threshold sample (cells of 64 rows, their two best scores), the candidate
    lists start empty and the main launch scans ALL rows.  The pass needs a sample of at most half the corpus and 4 x rank <= cells: on
    128 compute units (64 chunk streams x one tile = 16384 rows, 256 cells) k = 64 is the depth at which rank (63) < k still holds."""
    engine = dense_opts
    n, d, b, k = 40000, 256, 512, 64
    assert _seed_rank(k, 16384, n) == 63
    x, q16, e, dl = _data(n, d, b)
    engine.set_option("n_cus", 128)
    engine.set_option("dense_gemv", 0)
    engine.set_dense(x)
    _check_call(engine, x, q16, e, dl, k, True, what="sample pass")
    assert engine.stat("dense_sample_passes") == 2                    # (the EXACT and the FAST call)


def test_failed_speculation_sets_its_bit(dense_opts):
    """The premise-breaking construction of test_dense_speculation_failure_is_caught, at its size: with the caller's order kept, the first
    rows are exactly what the queries ask for, the threshold lands far above the true k-th best, and the oracle says that fewer than k rows
    can reach the verification level -- bit 8 must be set for every query.  With the row placement on, every query is comfortable."""
    engine = dense_opts
    rng = np.random.default_rng(77)
    n, d, b, k = 40000, 256, 6, 60
    topic = rng.standard_normal(d)
    x32 = rng.standard_normal((n, d))
    x32[:40] = topic + 0.2 * rng.standard_normal((40, d))
    x = to_f16_unit(x32)
    q16 = to_f16_unit(topic + 0.2 * rng.standard_normal((b, d)))
    e, dl = exact_scores(x, q16), delta_of(x, q16)
    engine.set_option("dense_n0", 512)
    engine.set_option("dense_gemv", 0)
    assert speculative(k, 512, n)
    engine.set_option("dense_shuffle", 0)
    engine.set_dense(x)
    tau, cnt, flag = _check_call(engine, x, q16, e, dl, k, True, want_comfortable=False, what="speculation fails")
    for i in range(b):
        assert bands(e[i], tau[i], dl[i], k)["n_lo"] < k              # the premise of this case, from the oracle
    assert np.all(flag & FLAG_SPECULATION), flag                      # (asserted per query inside _check_call too)
    engine.set_option("dense_shuffle", 1)
    engine.set_dense(x)
    tau, cnt, flag = _check_call(engine, x, q16, e, dl, k, True, what="speculation holds")
    assert not np.any(flag)


def test_constructed_overflows_set_their_bits(dense_opts):
    """20000 exact copies of the chunk query 0 asks for: L > 16384, the candidate list must overflow (bit 1).  3000 exact copies of what
    query 1 asks for: the list holds them (U <= 16384) but all 3000 tie at the k-th score, more than the 2048-entry gather (bit 2).  The
    three plain queries are comfortable and unflagged; the counter equals the flagged queries; the answers are the oracle's."""
    engine = dense_opts
    rng = np.random.default_rng(41)
    n, d, k = 30000, 128, 60
    x = to_f16_unit(rng.standard_normal((n, d)))
    hot, near = to_f16_unit(rng.standard_normal((2, d)))
    copies = np.sort(rng.choice(n, size=20000, replace=False))
    x[copies] = hot
    x[np.setdiff1d(np.arange(n), copies)[:3000]] = near
    q16 = np.stack([hot, near] + list(to_f16_unit(rng.standard_normal((3, d)))))
    b = q16.shape[0]
    e, dl = exact_scores(x, q16), delta_of(x, q16)
    n0 = 4096                                                         # (the copies reach the lists through the seed select AND the scan)
    engine.set_option("dense_n0", n0)
    engine.set_dense(x)
    engine.reset_stats()
    ids, sc, ln = engine.dense_topk(q16, k)
    tau, cnt, flag = engine.dense_query_state(b)
    want_list, want_gather = [], []
    for i in range(b):
        bd = bands(e[i], tau[i], dl[i], k)
        ties = int(np.count_nonzero(e[i] >= bd["kth"]))
        tag = f"query {i}: tau {tau[i]!r} cand_cnt {cnt[i]} flag {flag[i]} ties {ties} {bd}"
        if bd["L"] > LIST_CAP:
            want_list.append(i)
            assert flag[i] & FLAG_LIST, tag
        elif bd["U"] <= LIST_CAP and ties > GATHER_CAP:               # every row with E >= kth has fp32 >= fp32-kth - 2 delta: gathered
            want_gather.append(i)
            assert flag[i] & FLAG_GATHER, tag
        elif comfortable(bd, k, speculative(k, n0, n)):
            assert flag[i] == 0, tag
    assert want_list == [0] and want_gather == [1] and np.count_nonzero(flag) == 2, (want_list, want_gather, flag)
    assert engine.stat("dense_exhaustive_queries") == 2 and engine.dense_diag()["exhaustive"] == 2
    for i in range(b):
        oid, osc = dense_exact_topk(x, q16[i], k)
        assert np.array_equal(ids[i], oid) and np.array_equal(sc[i].view(np.uint64), osc.view(np.uint64)), i


# ---- (c) guaranteed thresholds are not verified -------------------------------------------------------------------------------------
BLOCKS = [9000, 3000, 40, 40000]                                      # inside / beyond the 4096-row prefix, fewer rows than k, a long block
_BLOCK_DATA = {}


def _block_data():
    if not _BLOCK_DATA:
        n, d, b = sum(BLOCKS), 256, 64
        x = synth.dense_corpus(n, d, seed=2301)
        q16 = to_f16_unit(synth.dense_queries(x, b, seed=2302))
        dir_id = np.repeat(np.arange(len(BLOCKS)), BLOCKS).astype(np.int16)
        e, dl = exact_scores(x, q16), delta_of(x, q16)
        for a in (x, q16, dir_id, e, dl):
            a.setflags(write=False)
        _BLOCK_DATA["v"] = (x, q16, dir_id, e, dl)
    return _BLOCK_DATA["v"]


def _check_unflagged(engine, x, q16, e, dl, k, filt, dir_id, n0, oracle_rows, what):
    """After a dense call: every query comfortable by the oracle (so zero flags are PROVABLE), no flag, and the oracle's lists."""
    b = q16.shape[0]
    ids, sc, ln = engine.dense_topk(q16, k, filter_dir=filt)
    tau, cnt, flag = engine.dense_query_state(b)
    st = engine.stats()
    print(f"{what}: {np.count_nonzero(flag)} of {b} queries flagged, dense_exhaustive_queries {st['dense_exhaustive_queries']}, "
          f"dense_group_reruns {st['dense_group_reruns']}")           # (the figures, before anything is asserted)
    for i in range(b):
        mask = None if filt is None or filt[i] < 0 else dir_id == filt[i]
        ea = e[i] if mask is None else e[i][mask]
        nv = ea.shape[0]
        spec = speculative(k, n0, nv)
        bd = bands(ea, tau[i], dl[i], k)
        tag = f"{what} query {i} (view of {nv} rows, {'speculative' if spec else 'guaranteed'}): tau {tau[i]!r} cand_cnt {cnt[i]} flag {flag[i]} {bd}"
        assert comfortable(bd, k, spec), "badly chosen case: " + tag
        if nv <= min(n0, 32768):                                      # a whole-view threshold: zero flags follow from the oracle alone
            assert bd["U"] <= bd["W"] <= 1024, tag
        assert bd["L"] <= cnt[i] <= bd["U"], tag
        assert flag[i] == 0, tag
    for i in oracle_rows:
        mask = None if filt is None or filt[i] < 0 else dir_id == filt[i]
        oid, osc = dense_exact_topk(x, q16[i], k, mask)
        assert ln[i] == len(oid) and np.array_equal(ids[i, :ln[i]], oid), (what, i)
        assert np.array_equal(sc[i, :ln[i]].view(np.uint64), osc.view(np.uint64)), (what, i)
    return st


@pytest.mark.parametrize("group_sample", [1, 0], ids=["group-sample", "store-kernel-seed"])
@pytest.mark.parametrize("k,n0", [(60, 4096), (288, 4096), (1, 4096), (2, 4096), (3, 4096), (60, 32768), (288, 32768)])
def test_grouped_launch_does_not_verify_guaranteed_bounds(dense_opts, k, n0, group_sample):
    """Four block groups in ONE launch per stage; a view whose seed rank is k carries a GUARANTEED bound: its k-th prefix score, nudged
    up, is reached by at most k - 1 candidates of a whole-view prefix, so a final kernel that "verifies" it flags the query and the group
    is run again -- exact answers, double work.  No query may be flagged, nothing re-run.
      dense_n0 = 4096: the 3000-row block (inside the prefix; at k = 288 the list is nearly the block) and the 40-row block (fewer rows than
                       k) are whole-view thresholds, the 9000-row block's rank (65 at k = 60) reaches k, the 40000-row block is speculative
                       at k = 60 / 288 (and verified) and guaranteed at k <= 3;
      dense_n0 = 32768 (the default): the 9000-row block lies inside the prefix too, and the long block's rank reaches k."""
    engine = dense_opts
    x, q16, dir_id, e, dl = _block_data()
    n, b = x.shape[0], q16.shape[0]
    filt = (np.arange(b) % len(BLOCKS)).astype(np.int16)
    engine.set_option("dense_n0", n0)
    engine.set_option("dense_dir_blocks", 2)
    engine.set_option("dense_dir_block_min_rows", 1)
    engine.set_option("dense_group_sample", group_sample)
    engine.set_dense(x)
    engine.set_doc_meta(n, None, dir_id)
    try:
        engine.dense_topk(q16[:4], k, filter_dir=filt[:4])           # (builds the block copies: the counters below see one call)
        engine.reset_stats()
        st = _check_unflagged(engine, x, q16, e, dl, k, filt, dir_id, n0, range(0, b, 5), f"grouped k={k} n0={n0} group_sample={group_sample}")
        diag = engine.dense_diag()
        assert st["dense_exhaustive_queries"] == 0 and st["dense_group_reruns"] == 0, st
        assert st["dense_grouped_launches"] == 1 and st["dense_block_groups"] == 4, st
        assert diag["exhaustive"] == 0 and diag["uncertified"] == 0, diag
    finally:
        engine.set_doc_meta(n, None, None)


@pytest.mark.parametrize("block,k", [(0, 60), (1, 288), (2, 60), (3, 2)])
def test_single_block_group_does_not_verify_guaranteed_bounds(dense_opts, block, k):
    """One block group: the view path of the ordinary pipeline (no grouped launch), same four views."""
    engine = dense_opts
    x, q16, dir_id, e, dl = _block_data()
    n, b, n0 = x.shape[0], 16, 4096
    filt = np.full(b, block, np.int16)
    engine.set_option("dense_n0", n0)
    engine.set_option("dense_dir_blocks", 2)
    engine.set_option("dense_dir_block_min_rows", 1)
    engine.set_dense(x)
    engine.set_doc_meta(n, None, dir_id)
    try:
        engine.dense_topk(q16[:1], k, filter_dir=filt[:1])
        engine.reset_stats()
        st = _check_unflagged(engine, x, q16[:b], e[:b], dl[:b], k, filt, dir_id, n0, (0, b - 1), f"single group block {block} k={k}")
        assert st["dense_exhaustive_queries"] == 0 and st["dense_group_reruns"] == 0, st
        assert st["dense_grouped_launches"] == 0 and st["dense_block_groups"] == 1, st
    finally:
        engine.set_doc_meta(n, None, None)


@pytest.mark.parametrize("k", [288, 1])
def test_unrouted_view_inside_the_prefix_is_not_verified(dense_opts, k):
    """An unrouted corpus with N <= n0 (the 3000 rows of block 1 on their own)."""
    engine = dense_opts
    x, q16, dir_id, e, dl = _block_data()
    rows = np.flatnonzero(dir_id == 1)
    xs, es = np.ascontiguousarray(x[rows]), e[:, rows]
    b = 16
    engine.set_dense(xs)
    engine.reset_stats()
    st = _check_unflagged(engine, xs, q16[:b], es[:b], delta_of(xs, q16[:b]), k, None, None, 32768, (0, b - 1), f"unrouted k={k}")
    assert st["dense_exhaustive_queries"] == 0 and engine.dense_diag()["exhaustive"] == 0
