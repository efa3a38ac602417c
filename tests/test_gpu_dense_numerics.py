"""GPU, dense route on the inputs its other tests never produce (tests/dense_numerics_util.py): all-negative scores, zero rows and a zero
query, fp16 subnormals in either operand, row norms spread over 2^8, scores that cancel to a few delta, and the fp32 -> fp16 conversion at its
edges.  Wherever a path returns an EXACT answer: ids and fp64 score bits equal oracle.dense_exact_topk (masked where filtered), lengths are
right, padding is id -1 / score 0.  Wherever a pruned pipeline ran: its state (threshold, candidate count, flags) is held against counts from
fp64 scores, as in test_gpu_dense_pruning.py.  Every tolerance is dense_pruning_util's dh = 1.01 delta, or bit equality.

The scenes' own preconditions (what makes a defect visible) are asserted in test_dense_numerics_cpu.py, without a GPU."""
import numpy as np
import pytest

import dense_numerics_util as scenes
from dense_pruning_util import (FLAG_LIST, LIST_CAP, SCAN_ARM_IDS, SCAN_ARMS, apply_scan_arm, bands, check_fast_ranking, comfortable, delta_hat,
                                delta_of, exact_scores, reset_scan_arm, speculative)
from easyrag_amd import _lib
from easyrag_amd.engine import queries_to_csr
from easyrag_amd.index import BM25S, build_bm25_index
from oracle import BM25SLucene, bm25_filter, dense_exact_topk, reciprocal_rank_fusion
from oracle.dense import dense_exact_scores
from oracle.retrievers import Item

pytestmark = pytest.mark.gpu

_BUILDERS = {"negative": scenes.negative_scene, "zeros": scenes.zeros_scene, "subnormal": scenes.subnormal_scene,
             "subnormal-queries": scenes.subnormal_queries_scene, "range": scenes.range_scene, "cancellation": scenes.cancellation_scene,
             "negative-dirs": scenes.negative_dirs_scene, "subnormal-dirs": scenes.subnormal_dirs_scene,
             "negative-80037": scenes.negative_big_scene, "zeros-80037": scenes.zeros_big_scene, "subnormal-80037": scenes.subnormal_big_scene}
_SCENES = {}
_BIG = None                       # the one 80037-row scene kept in memory
_ORACLE_CACHE = {}                # (scene, query) -> the oracle's pinned-order fp64 score vector: the arms and the masked rankings share it
_E_CACHE = {}                     # (scene, query) -> (E[q, :], delta(q))


def _scene(name):
    """(x16, q16, k, extras) of a scene: built once, shared, never written to."""
    global _BIG
    if name not in _SCENES:
        if name.endswith("80037"):
            if _BIG is not None:
                _SCENES.pop(_BIG)
                for cache in (_ORACLE_CACHE, _E_CACHE):
                    for key in [key for key in cache if key[0] == _BIG]:
                        del cache[key]
            _BIG = name
        x, q, k, extras = _BUILDERS[name]()
        x.setflags(write=False)
        q.setflags(write=False)
        _SCENES[name] = (x, q, k, extras)
    return _SCENES[name]


def _oracle_scores(name, i):
    key = (name, int(i))
    if key not in _ORACLE_CACHE:
        x, q, _, _ = _scene(name)
        _ORACLE_CACHE[key] = dense_exact_scores(x, q[i])
    return _ORACLE_CACHE[key]


def _oracle_topk(name, i, k, mask=None):
    """oracle.dense_exact_topk(x, q[i], k, mask) from the cached score vector (rank_scores is held against it in test_dense_numerics_cpu.py)."""
    return scenes.rank_scores(_oracle_scores(name, i), k, mask)


def _e(name, i):
    key = (name, int(i))
    if key not in _E_CACHE:
        x, q, _, _ = _scene(name)
        _E_CACHE[key] = (exact_scores(x, q[i])[0], float(delta_of(x, q[i])[0]))
    return _E_CACHE[key]


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _assert_exact(name, i, ids, sc, ln, k, mask=None, what=""):
    """Row of an EXACT answer against the oracle: ids, fp64 score bits, length, padding."""
    oid, osc = _oracle_topk(name, i, k, mask)
    tag = f"{what} {name} query {i}"
    assert ln == len(oid), f"{tag}: length {ln} != {len(oid)}"
    assert np.array_equal(ids[:ln], oid), f"{tag}: ids differ at {np.flatnonzero(ids[:ln] != oid)[:5]}: {ids[:ln][ids[:ln] != oid][:5]} != {oid[ids[:ln] != oid][:5]}"
    assert np.array_equal(_bits(sc[:ln]), _bits(osc)), f"{tag}: fp64 score bits differ"
    assert np.all(ids[ln:] == -1) and np.all(_bits(sc[ln:]) == 0), f"{tag}: padding is not (id -1, score +0.0)"


# ---- (a) fp32 scores against the bound --------------------------------------------------------------------------------------------
def _score_case(name):
    base, _, cut = name.partition("/")
    x, q, k, extras = _scene(base)
    if cut == "d64":
        x, q = np.ascontiguousarray(x[:, :64]), np.ascontiguousarray(q[:, :64])
    elif cut == "twin":
        x, q = scenes.range_twin(x, q, extras)
    b = 70
    rows = list(range(b - 1)) + [extras.get("zero_query", b - 1)]
    return x, q[rows]


@pytest.mark.parametrize("name", ["negative", "zeros", "subnormal", "subnormal-queries", "range", "range/twin", "cancellation",
                                  "negative/d64", "range/d64"])
def test_fp32_scores_lie_within_the_bound(engine, name):
    """The store kernel (MFMA) and the plain kernel against fp64 within dh = 1.01 d 2^-23 |q| max|x| -- the bound the pruning margins rest on,
    here with |q| max|x| from 0 (the zero query: the scores must BE zero) over 1e-3 (subnormal queries) to 2^17 (the scaled twin), and with
    subnormal operands: an instruction that flushes them is off by >= 10 delta (the scenes' precondition).  70 queries, all rows plus a
    ragged range at the end of the matrix."""
    x, q = _score_case(name)
    n = x.shape[0]
    engine.set_dense(x)
    ref = exact_scores(x, q)
    dh = delta_hat(x, q)[:, None]
    for row0, rows in ((0, n), (n - 301, 301)):
        want = ref[:, row0:row0 + rows]
        for use_mfma in (False, True):
            got = engine.debug_dense_scores(q, row0, rows, use_mfma=use_mfma)
            err = np.abs(got - want)
            worst = float(np.max(err / np.maximum(dh, 1e-300)))
            print(f"{name} rows {row0}+{rows} mfma={use_mfma}: max |fp32 - fp64| / dh = {worst:.3g}")
            assert np.all(err <= dh), (name, row0, use_mfma, worst)


# ---- (b) every scan arm -----------------------------------------------------------------------------------------------------------
@pytest.fixture(params=SCAN_ARMS, ids=SCAN_ARM_IDS)
def arm(request, engine):
    """Every dense-scan kernel of the library (dense_pruning_util.SCAN_ARMS); guaranteed bounds refined in stages (dense_n0 = 512, dense_n1 =
    2048), speculative thresholds from a 1024-row prefix."""
    apply_scan_arm(engine, request.param)
    engine.set_option("dense_n0", 1024 if request.param[4] else 512)
    engine.set_option("dense_n1", 2048)
    try:
        yield request.param
    finally:
        reset_scan_arm(engine)
        engine.set_option("dense_n0", 32768)
        engine.set_option("dense_n1", 131072)


BATCHES = (5, 40, 200)            # the skinny-GEMM stream, the half query tile, the full tile


def _batch(extras, b):
    """Query rows of a batch of b: the first b, the zero query (zeros scene) in the last place."""
    rows = np.arange(b)
    if "zero_query" in extras:
        rows[-1] = extras["zero_query"]
    return rows


def _sample(b):
    return sorted(set([0, 1, 2, 3, b - 1] + ([100, 101] if b > 101 else [])))


def _check_pruned_call(engine, name, rows, arm, twin=None):
    """One EXACT and one FAST call on the scene's queries `rows` with the engine's current options and matrix; parity, pruning state and the
    FAST ranking of the sampled queries.  Returns the EXACT result."""
    x, q, k, extras = _scene(name)
    n, b = x.shape[0], len(rows)
    qb = np.ascontiguousarray(q[rows])
    n0 = engine.get_option("dense_n0")
    spec = bool(arm[4]) and speculative(k, n0, n)
    staged = not spec and n0 < engine.get_option("dense_n1") < n      # tau is the last stage's: it does not bound an earlier stage's list
    engine.reset_stats()
    ids, sc, ln = engine.dense_topk(qb, k, mode=_lib.ERH_DENSE_EXACT)
    diag = engine.dense_diag()
    tau, cnt, flag = engine.dense_query_state(b)
    exhaustive = engine.stat("dense_exhaustive_queries")
    fids, fsc, fln = engine.dense_topk(qb, k, mode=_lib.ERH_DENSE_FAST)
    what = f"{name} B={b} arm={arm}"
    assert diag["uncertified"] == 0 and diag["max_abs_err"] <= diag["margin"], (what, diag)
    assert exhaustive == int(np.count_nonzero(flag)) == diag["exhaustive"], (what, exhaustive, diag, flag)
    assert np.all(ln == k) and np.all(fln == k), what
    if name == "cancellation":                                        # W > 1024 for every query: the exhaustive path answers all of them
        assert np.all(flag != 0) and diag["exhaustive"] == b, (what, flag, diag)
    n_checked = n_comfortable = 0
    for j in _sample(b):
        i = int(rows[j])
        _assert_exact(name, i, ids[j], sc[j], ln[j], k, what=what)
        if i == extras.get("zero_query", -1):
            continue                                                  # delta = 0: only its answer is checked
        e, dl = _e(name, i)
        bd = bands(e, tau[j], dl, k)
        tag = f"{what} query {i}: tau {tau[j]!r} cand_cnt {cnt[j]} flag {flag[j]} {bd}"
        assert np.isfinite(tau[j]) or tau[j] == -np.inf, tag
        ok = comfortable(bd, k, spec)
        n_checked += 1
        n_comfortable += ok
        if ok:
            assert (int(flag[j]) & ~(FLAG_LIST if staged else 0)) == 0, "flagged although comfortable: " + tag
        if not staged and cnt[j] <= LIST_CAP:
            assert bd["L"] <= cnt[j] <= bd["U"], tag
        check_fast_ranking(fids[j, :fln[j]], fsc[j, :fln[j]], e, None, k, bd["dh"], what=f"{what} query {i} (FAST)")
    if name != "cancellation":                                        # a badly chosen case fails; it cannot pass vacuously
        assert 4 * n_comfortable >= 3 * n_checked, f"{what}: only {n_comfortable} of {n_checked} sampled queries are comfortable"
    return ids, sc, ln


@pytest.mark.parametrize("name", ["negative", "zeros", "subnormal", "subnormal-queries", "range", "cancellation"])
def test_every_scan_arm(engine, arm, name):
    """EXACT and FAST at 5, 40 and 200 queries on every arm.  Negative / zeros: a phantom score of 0 (a row past N in the last tile of
    8037 = 31 x 256 + 101 rows, an empty slot, a padding entry) would outrank every real row of an anti query; the 80 zero rows must lead with
    +0.0 in index order.  Subnormal scenes: a flushed operand moves scores by >= 10 delta and prunes true members.  Cancellation: every query
    exceeds the re-score budget and is answered by the exhaustive path.  Range: the scaled twin gives the same ids and 2^9 x the scores."""
    x, q, k, extras = _scene(name)
    engine.set_dense(x)
    got = {b: _check_pruned_call(engine, name, _batch(extras, b), arm) for b in BATCHES}
    if name == "range":
        xt, qt = scenes.range_twin(x, q, extras)
        engine.set_dense(xt)
        for b in BATCHES:
            ids, sc, ln = got[b]
            tids, tsc, tln = engine.dense_topk(np.ascontiguousarray(qt[:b]), k)
            assert engine.dense_diag()["uncertified"] == 0
            assert np.array_equal(tln, ln) and np.array_equal(tids, ids), f"B={b}: the scaled twin ranks differently"
            assert np.array_equal(_bits(tsc), _bits(np.ldexp(sc, 9))), f"B={b}: the scaled twin's scores are not 2^9 x the scores"


# ---- (c) batches padded to >= 512 queries -----------------------------------------------------------------------------------------
@pytest.fixture
def big_opts(engine):
    yield engine
    for name, value in (("dense_tile384", 1), ("dense_selfseed", 1), ("n_cus", 0)):
        engine.set_option(name, value)


def _device_cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _sample_pass_qualifies(cus, bpad, n, k, n0):
    """The pipeline's own rule (pipeline_dense.hip) for an unfiltered batch padded to bpad >= 512 queries on `cus` compute units: 8 chunk
    streams per (8 x query tiles) CUs, one 256-row tile per stream (more only below 16384 sampled rows), four 64-row cells per tile; the pass
    needs N >= 2 x sampled rows, a speculative rank, and 4 x rank <= cells."""
    n_qt = bpad // 256
    streams = cus // (8 * n_qt) * 8
    if streams <= 0:
        return False
    seed_tiles = max(1, min(n0, 16384) // (streams * 256))
    rows_seed = seed_tiles * streams * 256
    if rows_seed > n:
        return False
    rank = int(_lib.load().erh_dense_seed_rank(k, rows_seed, n))
    return n >= 2 * rows_seed and rank < k and 4 * rank <= seed_tiles * streams * 4


@pytest.mark.parametrize("name", ["negative-80037", "zeros-80037", "subnormal-80037"])
def test_600_queries_sample_pass_and_384_row_tile(big_opts, name):
    """600 queries (three query tiles) on 80037 = 208 x 384 + 165 = 312 x 256 + 165 rows: with the default options, then dense_tile384 0 / 1 x
    dense_selfseed 0 / 1 on 128 compute units (40 chunk streams: a sample of 10240 rows, 160 cells, rank 40).  The default call is held to the
    same counters: on the device's own CU count (256: 80 streams, 20480 rows, 320 cells, rank 62) the pass qualifies by the pipeline's rule.  The sample pass scores whole tiles WITHOUT a threshold and keeps the two best of every 64-row cell: a zero row past N
    would be the best of its cell for every anti query and lift the threshold to 0 - margin, above every real row.  The counters prove which
    kernels ran; the sampled queries equal the oracle and, comfortable by the oracle, are not flagged."""
    engine = big_opts
    x, q, k, extras = _scene(name)
    n, b = x.shape[0], q.shape[0]
    assert b == 600 and int(_lib.load().erh_dense_seed_rank(k, 10240, n)) == 40
    engine.set_dense(x)
    first = None
    for tile384, selfseed, n_cus in ((1, 1, 0), (1, 1, 128), (1, 0, 128), (0, 1, 128), (0, 0, 128)):
        engine.set_option("dense_tile384", tile384)
        engine.set_option("dense_selfseed", selfseed)
        engine.set_option("n_cus", n_cus)
        what = f"{name} tile384={tile384} selfseed={selfseed} n_cus={n_cus}"
        engine.reset_stats()
        ids, sc, ln = engine.dense_topk(q, k)
        st = engine.stats()
        diag = engine.dense_diag()
        tau, cnt, flag = engine.dense_query_state(b)
        print(f"{what}: pp5 {st['dense_scan_pp5_launches']} pp3 {st['dense_scan_pp3_launches']} sample passes {st['dense_sample_passes']} "
              f"flagged {np.count_nonzero(flag)} exhaustive {diag['exhaustive']}")
        assert diag["uncertified"] == 0 and diag["max_abs_err"] <= diag["margin"], (what, diag)
        # the default call (n_cus = 0: every CU of the device) must take the sample pass and the 384-row tile like the pinned ones
        assert _sample_pass_qualifies(n_cus or _device_cus(), 768, n, k, engine.get_option("dense_n0")), \
            f"{what}: the sample pass cannot qualify on {n_cus or _device_cus()} compute units -- the scene's size was chosen for 128 .. 256"
        assert st["dense_sample_passes"] == selfseed, (what, st)
        assert (st["dense_scan_pp5_launches"] >= 1) == bool(tile384) and (tile384 or st["dense_scan_pp3_launches"] >= 1), (what, st)
        assert st["dense_scan_gemv_launches"] == 0 and st["dense_tile384_nomem"] == 0, (what, st)
        spec = bool(st["dense_sample_passes"]) or speculative(k, engine.get_option("dense_n0"), n)
        n_comfortable = 0
        for i in scenes.BIG_SAMPLE:
            _assert_exact(name, i, ids[i], sc[i], ln[i], k, what=what)
            if i == extras.get("zero_query", -1):
                continue
            e, dl = _e(name, i)
            bd = bands(e, tau[i], dl, k)
            tag = f"{what} query {i}: tau {tau[i]!r} cand_cnt {cnt[i]} flag {flag[i]} {bd}"
            ok = comfortable(bd, k, spec)
            n_comfortable += ok
            assert not ok or flag[i] == 0, "flagged although comfortable: " + tag
            assert bd["L"] <= cnt[i] <= bd["U"], tag
        assert n_comfortable >= 6, f"{what}: only {n_comfortable} sampled queries are comfortable"
        if first is None:
            first = (ids, sc, ln)
        else:                                                         # every query of the batch, not only the sampled ones
            assert np.array_equal(ids, first[0]) and np.array_equal(_bits(sc), _bits(first[1])) and np.array_equal(ln, first[2]), what


# ---- (d) dir filter ---------------------------------------------------------------------------------------------------------------
@pytest.fixture
def dir_opts(engine):
    yield engine
    for name, value in (("dense_dir_blocks", 1), ("dense_group_launch", 1), ("dense_group_sample", 1)):
        engine.set_option(name, value)


@pytest.mark.parametrize("name", ["negative-dirs", "subnormal-dirs"])
def test_dir_filter_blocks_grouped_launch_and_filter_column(dir_opts, name):
    """37 queries with filters -1 / 0 / 1 on two classes of 4600 and 4401 rows (per-dir block copies: both end inside a tile, and the zero
    rows behind a block are not rows of the class): the filter column, and the block route with the grouped launch / its own sample pass on and
    off, equal each other on every query and the masked oracle on the sampled ones."""
    engine = dir_opts
    x, q, k, extras = _scene(name)
    n, b = x.shape[0], 37
    dir_id = extras["dir_id"]
    qb = np.ascontiguousarray(q[:b])
    filt = (np.arange(b) % 3 - 1).astype(np.int16)
    engine.set_dense(x)
    engine.set_doc_meta(n, None, dir_id)
    try:
        results = {}
        for blocks, group_launch, group_sample in ((0, 1, 1), (2, 1, 1), (2, 1, 0), (2, 0, 1), (2, 0, 0)):
            engine.set_option("dense_dir_blocks", blocks)
            engine.set_option("dense_group_launch", group_launch)
            engine.set_option("dense_group_sample", group_sample)
            engine.reset_stats()
            results[(blocks, group_launch, group_sample)] = engine.dense_topk(qb, k, filter_dir=filt)
            st, diag = engine.stats(), engine.dense_diag()
            what = f"{name} blocks={blocks} group_launch={group_launch} group_sample={group_sample}"
            print(f"{what}: groups {st['dense_block_groups']} grouped launches {st['dense_grouped_launches']} exhaustive {diag['exhaustive']}")
            assert diag["uncertified"] == 0, (what, diag)
            assert st["dense_block_groups"] == (2 if blocks else 0), (what, st)
            assert (st["dense_grouped_launches"] > 0) == bool(blocks and group_launch), (what, st)
        ids, sc, ln = results[(0, 1, 1)]
        for key, (i2, s2, l2) in results.items():
            assert np.array_equal(i2, ids) and np.array_equal(_bits(s2), _bits(sc)) and np.array_equal(l2, ln), f"{name} {key} differs from the filter column"
        for i in (0, 1, 2, 3, 4, 5, b - 1):
            mask = None if filt[i] < 0 else dir_id == filt[i]
            _assert_exact(name, i, ids[i], sc[i], ln[i], k, mask, what="dir filter")
    finally:
        engine.set_doc_meta(n, None, None)


# ---- (e) row lists ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["negative", "zeros", "subnormal"])
def test_row_lists_short_and_long(engine, name):
    """erh_dense_topk_rows: a list of at most 2048 rows (one launch) and a longer one (score + select), each holding zero rows and ordinary
    rows in the zeros scene, and one list shorter than k: its padding (id -1, score 0) must stay BEHIND the negative scores."""
    x, q, k, extras = _scene(name)
    n = x.shape[0]
    rng = np.random.default_rng(31)
    zr = extras.get("zero_rows", np.zeros(0, np.int64))
    lists = [np.union1d(zr[::2], rng.choice(n, size=1500, replace=False)), np.union1d(zr, rng.choice(n, size=3001, replace=False)),
             np.union1d(zr[:5], rng.choice(n, size=55, replace=False))]
    assert len(lists[0]) <= 2048 < len(lists[1]) and len(lists[2]) < k
    rows = _batch(extras, 9)
    list_of = np.arange(9) % 3
    engine.set_dense(x)
    engine.reset_stats()
    ids, sc, ln = engine.dense_topk_rows(np.ascontiguousarray(q[rows]), k, lists, list_of)
    assert engine.stat("dense_rows_calls") == 1 and engine.stat("dense_rows_short_launches") >= 1 and engine.stat("dense_rows_long_launches") >= 1
    for j, i in enumerate(rows):
        mask = np.zeros(n, bool)
        mask[lists[list_of[j]]] = True
        _assert_exact(name, int(i), ids[j], sc[j], ln[j], k, mask, what=f"row list {list_of[j]}")
        assert ln[j] == min(k, len(lists[list_of[j]]))


# ---- (f) set filters --------------------------------------------------------------------------------------------------------------
def test_set_filters_merge_negative_lists(engine):
    """erh_dense_topk_sets on the negative dirs scene: MatchAny of both classes (two sub-queries, merged), a single class, an empty set, no
    filter.  The merged list of an anti query holds negative scores only: no padding entry (id -1, score 0) in front of them."""
    name = "negative-dirs"
    x, q, k, extras = _scene(name)
    n, b = x.shape[0], 20
    dir_id = extras["dir_id"]
    sets = [([0, 1], [0], [1], [], None)[i % 5] for i in range(b)]
    engine.set_dense(x)
    engine.set_doc_meta(n, None, dir_id)
    try:
        engine.reset_stats()
        ids, sc, ln = engine.dense_topk_sets(np.ascontiguousarray(q[:b]), k, sets)
        assert engine.dense_diag()["uncertified"] == 0
    finally:
        engine.set_doc_meta(n, None, None)
    for i in range(b):
        mask = None if sets[i] is None else np.isin(dir_id, np.asarray(sets[i], np.int64))
        _assert_exact(name, i, ids[i], sc[i], ln[i], k, mask, what=f"set {sets[i]}")
        assert ln[i] == (0 if sets[i] == [] else k)
        assert np.all(ids[i, :ln[i]] >= 0)
        if i in extras["anti"]:
            assert np.all(sc[i, :ln[i]] < 0.0), f"query {i} (set {sets[i]}): a score of 0 among negative scores"


# ---- (g) fused call ---------------------------------------------------------------------------------------------------------------
VOCAB = 600


def _tokens(rng, n, lo=8, hi=30):
    p = 1.0 / np.arange(1, VOCAB + 1) ** 1.07
    p /= p.sum()
    return [list(map(int, rng.choice(VOCAB, size=int(rng.integers(lo, hi)), p=p))) for _ in range(n)]


def test_fused_call_on_negative_dense_scores(engine):
    """erh_hybrid_topk with hybrid_lazy 2 and 0 on the negative scene (k_dense 288, k_sparse 192, topk 10): both equal the oracle composition
    bm25_filter + dense_exact_topk + reciprocal_rank_fusion exactly.  The lazy final kernel ranks by counting inside 2 delta windows of
    negative fp32 scores and writes (id, rank) pairs; a padding entry taken for a row would enter the fusion with a rank."""
    name = "negative"
    x, q, _, extras = _scene(name)
    n, b, kd, ks, topk, K = x.shape[0], 24, 288, 192, 10, 60
    rng = np.random.default_rng(61)
    docs = _tokens(rng, n)
    queries = [[int(t) for t in rng.choice(docs[int(rng.integers(0, n))], size=5)] for _ in range(b)]
    idx = build_bm25_index(docs, BM25S)
    ora = BM25SLucene(k1=1.5, b=0.75).index(docs)
    csr = queries_to_csr([idx.tokens_to_ids(t) for t in queries])
    qb = np.ascontiguousarray(q[:b])
    engine.set_dense(x)
    engine.set_bm25(idx)
    engine.set_doc_meta(n, None, None)
    out, lazy_queries = {}, {}
    try:
        for lazy in (2, 0):
            engine.set_option("hybrid_lazy", lazy)
            engine.reset_stats()
            out[lazy] = engine.hybrid_topk(qb, *csr, k_dense=kd, k_sparse=ks, K=K, topk=topk)
            lazy_queries[lazy] = engine.stat("hybrid_lazy_queries")
            assert engine.dense_diag()["uncertified"] == 0
    finally:
        engine.set_option("hybrid_lazy", 1)
        engine.free_bm25_slot(0)                                      # the shared engine keeps no index of this corpus
    assert lazy_queries[2] > 0 and lazy_queries[0] == 0, lazy_queries
    for i in range(b):
        A = [Item(j, int(j), s) for j, s in bm25_filter(ora.get_scores(queries[i]), ks, None)]
        D = [Item(int(j), int(j), float(s)) for j, s in zip(*_oracle_topk(name, i, kd))]
        if i in extras["anti"]:
            assert all(w.score < 0.0 for w in D)
        want = reciprocal_rank_fusion([A, D], K=K, topk=topk)
        for lazy in (2, 0):
            ids, sc, ln = out[lazy]
            assert ln[i] == len(want), (lazy, i)
            assert list(ids[i, :ln[i]]) == [w.idx for w in want], f"hybrid_lazy={lazy} query {i}: fused ids differ"
            assert list(sc[i, :ln[i]]) == [w.score for w in want], f"hybrid_lazy={lazy} query {i}: fused scores differ"


# ---- (i) conversions --------------------------------------------------------------------------------------------------------------
def test_fp32_rows_and_queries_round_like_numpy(engine):
    """convert_rows_kernel and prep_queries_kernel against numpy's round-to-nearest-even: halfway points between fp16 neighbours in the
    normal and the subnormal range, values below 2^-25, -0.0, 65504 and 65519 (the last fp32 integers in front of the overflow edge)."""
    x32 = scenes.conversion_matrix()
    n, d = x32.shape
    want = x32.astype(np.float16)
    engine.set_dense(x32, normalize=False)
    got = engine.get_dense_rows(0, n)
    bad = np.flatnonzero(got.view(np.uint16) != want.view(np.uint16))
    assert bad.size == 0, [(float(x32.reshape(-1)[i]), hex(got.view(np.uint16).reshape(-1)[i]), hex(want.view(np.uint16).reshape(-1)[i])) for i in bad[:8]]
    # the same matrix as fp32 queries, taken as they are: the answers are the oracle's on the numpy-rounded queries
    k = 10
    ids, sc, ln = engine.dense_topk_rows(x32, k, [np.arange(n)], np.zeros(n, np.int32), normalize_q=False)
    for i in range(n):
        oid, osc = dense_exact_topk(want, want[i], k)
        assert ln[i] == k and np.array_equal(ids[i], oid) and np.array_equal(_bits(sc[i]), _bits(osc)), i


def test_normalised_zero_row_and_zero_query(engine):
    """normalize = 1: an all-zero fp32 row is stored as zeros (no 0 / 0), an all-zero fp32 query is answered like the zero query of the zeros
    scene: every score 0, the first k rows in index order."""
    rng = np.random.default_rng(71)
    n, d, k = 300, 64, 10
    x32 = rng.standard_normal((n, d)).astype(np.float32)
    x32[5] = 0.0
    x32[n - 1] = -0.0
    engine.set_dense(x32, normalize=True)
    got = engine.get_dense_rows(0, n)
    assert np.all(np.isfinite(got)) and np.all(got[5].view(np.uint16) == 0) and np.all(got[n - 1].view(np.uint16) % 0x8000 == 0)
    q32 = rng.standard_normal((3, d)).astype(np.float32)
    q32[1] = 0.0
    ids, sc, ln = engine.dense_topk(q32, k, normalize_q=True)
    assert engine.dense_diag()["uncertified"] == 0
    assert ln[1] == k and np.array_equal(ids[1], np.arange(k)) and np.all(_bits(sc[1]) == 0)


# ---- non-finite rows are refused --------------------------------------------------------------------------------------------------
def test_non_finite_rows_are_refused(engine):
    """erh_set_dense refuses a matrix with an fp16 Inf or NaN, and an fp32 matrix with a value that converts to Inf (|v| >= 65520 with
    normalize = 0); the handle is then without a chunk matrix (a dense call fails as before any erh_set_dense), and a valid matrix works."""
    x, q, k, _ = _scene("negative")
    small = np.ascontiguousarray(x[:1001])
    try:
        for what, value in (("inf", np.inf), ("-inf", -np.inf), ("nan", np.nan)):
            bad = small.copy()
            bad[777, 13] = np.float16(value)
            engine.set_dense(small)
            with pytest.raises(_lib.ErhError, match="non-finite row") as err:
                engine.set_dense(bad)
            assert err.value.status == _lib.ERH_ERR_INVALID, what
            with pytest.raises(_lib.ErhError) as err:
                engine.dense_topk(np.ascontiguousarray(q[:3]), k)
            assert err.value.status == _lib.ERH_ERR_STATE, what
        for value in (65520.0, -1e30, np.inf):
            bad32 = small.astype(np.float32)
            bad32[1000, 255] = value
            with pytest.raises(_lib.ErhError, match="non-finite row") as err:
                engine.set_dense(bad32, normalize=False)
            assert err.value.status == _lib.ERH_ERR_INVALID, value
        ok32 = small.astype(np.float32)
        ok32[1000, 255] = 65519.0                                     # the largest magnitudes that still round to a finite fp16
        ok32[0, 0] = -65519.0
        engine.set_dense(ok32, normalize=False)
        assert np.array_equal(engine.get_dense_rows(0, 1001).view(np.uint16), ok32.astype(np.float16).view(np.uint16))
    finally:
        engine.set_dense(x)                                           # a valid matrix again, whatever happened
    ids, sc, ln = engine.dense_topk(np.ascontiguousarray(q[:6]), k)
    for i in range(6):
        _assert_exact("negative", i, ids[i], sc[i], ln[i], k, what="after the refusals")
