"""GPU parity, sparse route over explicit per-query row lists (erh_bm25_topk_rows, csrc/bm25_rows.hip): query b ranks the rows of its list by
their BM25 score and nothing else.  Every listed row gets the library-order sum, so ids AND fp64 score bits must equal the oracle's masked
walk, `bm25_filter(get_scores(q), k, keep_mask)` with the list as the mask, on both kernel shapes (lists of at most 2048 rows: one launch;
longer: score + select), both variants, and the existing routes where they answer the same question.

The oracle's ranking of a list is computed here from ONE get_scores vector per (index, query) -- bm25_filter walks that vector in canonical
order, stops at the first score <= 0 and keeps the masked rows; `_rank` does the same on the listed rows alone and is held against it
literally in test_rank_helper_is_the_oracle -- so that a sweep over many lists does not walk 40 000 documents in Python per case."""
import numpy as np
import pytest

from easyrag_amd import _lib, synth
from easyrag_amd.engine import RetrievalEngine, live_device_bytes, queries_to_csr
from easyrag_amd.index import BM25S, OKAPI, build_bm25_index
from oracle import BM25Okapi, BM25SLucene, bm25_filter

pytestmark = pytest.mark.gpu

KS = (1, 10, 192, 1024)
N, VOCAB, NQ = 40009, 2000, 12          # three Okapi skip tiles (16384 documents), two bm25s tiles (32768); N is odd
STATS = ("bm25_rows_calls", "bm25_rows_short_launches", "bm25_rows_long_launches")


def _bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


def _oracle_for(variant, docs):
    return BM25Okapi(docs, k1=1.5, b=0.75, epsilon=0.25) if variant == OKAPI else BM25SLucene(k1=1.5, b=0.75).index(docs)


def _scores(ora, q, n):
    """The oracle's score vector over n documents, widened exactly to float64 (what the entry reports); no token: zeros."""
    if len(q) == 0:
        return np.zeros(n, np.float64)
    return np.asarray(ora.get_scores(list(q))).astype(np.float64)


def _rank(scores, rows, k):
    """The rows of `rows` (ascending) with a score > 0 under (score desc, row id asc), the first k."""
    rows = np.asarray(rows, np.int64)
    s = scores[rows]
    rows, s = rows[s > 0], s[s > 0]
    order = np.lexsort((rows, -s))[:k]
    return rows[order], s[order]


def _pick(rng, pool, length):
    pool = np.arange(pool, dtype=np.int64) if np.isscalar(pool) else np.asarray(pool, np.int64)
    if length >= pool.shape[0]:
        return pool.copy()
    return np.sort(rng.choice(pool, size=length, replace=False))


def _check(got, S_of, lists, list_of, k, B, who=""):
    ids, sc, ln = (np.asarray(a.cpu()) if hasattr(a, "cpu") else np.asarray(a) for a in got)
    assert ids.shape == (B, k) and sc.shape == (B, k) and ln.shape == (B,)
    for b in range(B):
        l = b if list_of is None else int(list_of[b])
        rows = np.zeros(0, np.int64) if l < 0 else lists[l]
        oid, osc = _rank(S_of(b), rows, k)
        assert ln[b] == len(oid), (who, b, int(ln[b]), len(oid))
        assert np.array_equal(ids[b, :ln[b]], oid), (who, b)
        assert np.array_equal(_bits(sc[b, :ln[b]]), _bits(osc)), (who, b)
        assert np.all(ids[b, ln[b]:] == -1) and np.all(sc[b, ln[b]:] == 0.0), (who, b)


def _stats(engine):
    return {n: engine.stat(n) for n in STATS}


def _moved(engine, before):
    after = _stats(engine)
    return {n: after[n] - before[n] for n in after}, after


_CORPORA = {}


def _corpus(variant):
    """Index, oracle, twelve 10-token queries and their score vectors [12 x N] (float64), computed once per variant."""
    if variant not in _CORPORA:
        flat, lens = synth.token_corpus(N, VOCAB, seed=2, mean_len=20)
        docs = [list(map(int, d)) for d in synth.split_docs(flat, lens)]
        ora = _oracle_for(variant, docs)
        idx = build_bm25_index(docs, variant)
        queries = [list(map(int, q)) for q in synth.token_queries(flat, lens, VOCAB, NQ, seed=9)]
        S = np.stack([_scores(ora, q, N) for q in queries])
        _CORPORA[variant] = dict(docs=docs, ora=ora, idx=idx, queries=queries, S=S)
    return _CORPORA[variant]


def _csr(idx, queries):
    return queries_to_csr([idx.tokens_to_ids(q) for q in queries])


@pytest.mark.parametrize("variant", [OKAPI, BM25S])
def test_rank_helper_is_the_oracle(variant):
    c = _corpus(variant)
    rng = np.random.default_rng(3)
    for j, length, k in ((0, 0, 10), (1, 1, 10), (2, 300, 50), (3, 2048, 192), (4, 20000, 1024), (5, N, 10)):
        rows = _pick(rng, N, length)
        mask = np.zeros(N, bool)
        mask[rows] = True
        want = bm25_filter(c["ora"].get_scores(c["queries"][j]), k, mask)
        gid, gsc = _rank(c["S"][j], rows, k)
        assert [w[0] for w in want] == list(gid) and np.array_equal(_bits([w[1] for w in want]), _bits(gsc)), (j, length)


@pytest.mark.parametrize("variant", [OKAPI, BM25S])
def test_parity_sweep(engine, variant):
    c = _corpus(variant)
    idx, S = c["idx"], c["S"]
    engine.set_bm25(idx)
    rng = np.random.default_rng(11 + variant)
    st = _stats(engine)
    for k in KS:
        lens = [0, 1, max(k - 1, 0), k, k + 1, 5, 300, 2047, 2048, 2049, 4097, 20000, N]
        B = len(lens)
        lists = [_pick(rng, N, L) for L in lens]
        qs = [c["queries"][b % NQ] for b in range(B)]
        got = engine.bm25_topk_rows(*_csr(idx, qs), k, lists)
        mv, st = _moved(engine, st)
        assert mv == {"bm25_rows_calls": 1, "bm25_rows_short_launches": 1, "bm25_rows_long_launches": 1}, mv
        _check(got, lambda b: S[b % NQ], lists, None, k, B, ("sweep", k))
        # the oracle's own answers exercise the tie-break and both sides of k
        if k == 192:
            oid, osc = _rank(S[8 % NQ], lists[8], 2048)
            assert len(oid) > k and len(np.unique(osc)) < len(osc)
    # lengths <= 2048 only: no long launch; > 2048 only: no short launch
    lists = [_pick(rng, N, L) for L in (0, 7, 2048, 900)]
    got = engine.bm25_topk_rows(*_csr(idx, c["queries"][:4]), 10, lists)
    mv, st = _moved(engine, st)
    assert mv == {"bm25_rows_calls": 1, "bm25_rows_short_launches": 1, "bm25_rows_long_launches": 0}, mv
    _check(got, lambda b: S[b], lists, None, 10, 4, "short only")
    lists = [_pick(rng, N, L) for L in (2049, 6000, N)]
    got = engine.bm25_topk_rows(*_csr(idx, c["queries"][:3]), 10, lists)
    mv, st = _moved(engine, st)
    assert mv == {"bm25_rows_calls": 1, "bm25_rows_short_launches": 0, "bm25_rows_long_launches": 1}, mv
    _check(got, lambda b: S[b], lists, None, 10, 3, "long only")


@pytest.mark.parametrize("variant", [OKAPI, BM25S])
def test_all_positive_lists_around_the_select_limit(engine, variant):
    """Lists made of rows that all score > 0: the select list's fill stands exactly at and around its limit after a step (2048 = two steps
    of 1024 appends), the case that broke the dense select once.  And lists without one positive row."""
    c = _corpus(variant)
    idx = c["idx"]
    engine.set_bm25(idx)
    q = [0, 1, 2]                                                          # three frequent terms: more than 10 000 documents score
    s = _scores(c["ora"], q, N)
    pos, non = np.flatnonzero(s > 0), np.flatnonzero(c["S"][0] <= 0)
    assert pos.shape[0] >= 4097 and non.shape[0] >= 3000
    rng = np.random.default_rng(5)
    lens = (2047, 2048, 2049, 3072, 3073, 4097)
    lists = [pos[:L] for L in lens] + [_pick(rng, pos, L) for L in lens]
    B = len(lists)
    for k in (1, 192, 1024):
        got = engine.bm25_topk_rows(*_csr(idx, [q] * B), k, lists)
        _check(got, lambda b: s, lists, None, k, B, ("all positive", k))
        assert np.all(np.asarray(got[2]) == k)
    lists = [non[:500], non[:3000]]
    ids, sc, ln = engine.bm25_topk_rows(*_csr(idx, [c["queries"][0]] * 2), 10, lists)
    assert list(ln) == [0, 0] and np.all(ids == -1) and np.all(sc == 0.0)


@pytest.mark.parametrize("variant", [OKAPI, BM25S])
def test_query_shapes(engine, variant):
    c = _corpus(variant)
    idx, ora, Q = c["idx"], c["ora"], c["queries"]
    engine.set_bm25(idx)
    rng = np.random.default_rng(21)
    long70 = sum((Q[j] for j in range(7)), [])                             # 70 tokens: more than one token chunk
    assert len(long70) == 70
    qs = [[], [VOCAB + 5, VOCAB + 6], Q[6] + Q[6], long70, Q[1], Q[2], long70, Q[3] + [Q[3][0]]]
    assert idx.tokens_to_ids(qs[1]).shape[0] == 0                         # all out of vocabulary: nothing is left to send
    Sq = [_scores(ora, [t for t in q if t < VOCAB], N) for q in qs]
    assert not np.array_equal(Sq[2], c["S"][6])                          # (a repeated token counts twice)
    lists = [_pick(rng, N, L) for L in (300, 5000, 2048, 1000, 700, 9000, 20000, 2049)]
    lo = np.arange(8, dtype=np.int32)
    lo[4] = -1                                                             # no rows
    st = _stats(engine)
    for k in (10, 192):
        got = engine.bm25_topk_rows(*_csr(idx, qs), k, lists, list_of=lo)
        mv, st = _moved(engine, st)
        assert mv == {"bm25_rows_calls": 1, "bm25_rows_short_launches": 1, "bm25_rows_long_launches": 1}, mv     # a batch mixing both shapes
        _check(got, lambda b: Sq[b], lists, lo, k, 8, ("shapes", k))
        assert got[2][0] == 0 and got[2][1] == 0 and got[2][4] == 0
    # 1030 queries sharing one 2049-row list
    B, k = 1030, 10
    shared = [_pick(rng, N, 2049)]
    got = engine.bm25_topk_rows(*_csr(idx, [Q[b % NQ] for b in range(B)]), k, shared, list_of=np.zeros(B, np.int32))
    mv, st = _moved(engine, st)
    assert mv == {"bm25_rows_calls": 1, "bm25_rows_short_launches": 0, "bm25_rows_long_launches": 1}, mv
    _check(got, lambda b: c["S"][b % NQ], shared, np.zeros(B, np.int32), k, B, "shared-1030")
    # ... and 1030 queries on short lists of their own
    lists = [_pick(rng, N, int(L)) for L in rng.integers(0, 400, B)]
    got = engine.bm25_topk_rows(*_csr(idx, [Q[b % NQ] for b in range(B)]), k, lists)
    _check(got, lambda b: c["S"][b % NQ], lists, None, k, B, "distinct-1030")


def test_long_shape_runs_in_chunks_when_the_work_space_is_small(engine):
    c = _corpus(OKAPI)
    idx = c["idx"]
    engine.set_bm25(idx)
    rng = np.random.default_rng(5)
    B, k = 9, 100
    lists = [_pick(rng, N, 20000), _pick(rng, N, 2049)]
    lo = (np.arange(B) % 2).astype(np.int32)
    csr = _csr(idx, [c["queries"][b] for b in range(B)])
    want = engine.bm25_topk_rows(*csr, k, lists, list_of=lo)
    _check(want, lambda b: c["S"][b], lists, lo, k, B, "one chunk")
    engine.set_option("bm25_rows_ws_mb", 0)                    # the minimum: one list of N rows -- 40009 doubles, one 20000-row span + ...
    try:
        st = _stats(engine)
        got = engine.bm25_topk_rows(*csr, k, lists, list_of=lo)
        mv, _ = _moved(engine, st)
        assert mv["bm25_rows_long_launches"] >= 4, mv
    finally:
        engine.set_option("bm25_rows_ws_mb", 256)
    for a, b in zip(want, got):
        assert np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))


@pytest.mark.parametrize("variant", [OKAPI, BM25S])
def test_tie_corpus(engine, variant):
    """16 distinct documents x 40: exact score ties across the whole corpus, ordered by row id."""
    rng = np.random.default_rng(4)
    base = [list(map(int, rng.integers(0, 12, size=rng.integers(3, 9)))) for _ in range(16)]
    docs = [base[i % 16] for i in range(640)]
    ora = _oracle_for(variant, docs)
    idx = build_bm25_index(docs, variant)
    engine.set_bm25(idx)
    queries = [[0, 1, 2], [5], [3, 3, 7, 11], [2, 9]]
    lists = [np.arange(640), _pick(rng, 640, 300), _pick(rng, 640, 41), np.arange(100, 200)]
    for k in (7, 100, 1024):
        got = engine.bm25_topk_rows(*_csr(idx, queries), k, lists)
        for b, q in enumerate(queries):
            mask = np.zeros(640, bool)
            mask[lists[b]] = True
            want = bm25_filter(ora.get_scores(q), k, mask)
            assert got[2][b] == len(want) and list(got[0][b, :len(want)]) == [w[0] for w in want], (k, b)
            assert np.array_equal(_bits(got[1][b, :len(want)]), _bits([w[1] for w in want])), (k, b)


def test_okapi_index_with_non_positive_payloads(engine):
    """rank-bm25's epsilon * average_idf floor is negative when most terms sit in most documents: sums do not grow monotonically, and a
    listed row whose sum is <= 0 is not returned.  The direct sum needs no sign check."""
    rng = np.random.default_rng(8)
    docs = []
    for _ in range(3000):
        doc = [t for t in range(6) if rng.random() < 0.8] or [0]
        doc += [int(t) for t in rng.integers(0, 6, size=rng.integers(0, 4))]
        doc += [6] * (rng.random() < 0.1) + [7] * (rng.random() < 0.1)
        docs.append(doc)
    ora = _oracle_for(OKAPI, docs)
    idx = build_bm25_index(docs, OKAPI)
    assert float(idx.payload.min()) < 0.0 < float(idx.payload.max())
    engine.set_bm25(idx)
    queries = [[0, 1, 7], [6, 7, 2, 2], [7], [3], [6, 0, 1, 2, 3, 4, 5]]
    lists = [np.arange(3000), _pick(rng, 3000, 2500), _pick(rng, 3000, 2048), _pick(rng, 3000, 100), _pick(rng, 3000, 1500)]
    Sq = [_scores(ora, q, 3000) for q in queries]
    for k in (5, 150):
        got = engine.bm25_topk_rows(*_csr(idx, queries), k, lists)
        _check(got, lambda b: Sq[b], lists, None, k, 5, ("negative", k))
    mask = np.zeros(3000, bool)
    mask[lists[1]] = True
    want = bm25_filter(ora.get_scores(queries[1]), 150, mask)                # the literal oracle once more
    assert list(got[0][1, :got[2][1]]) == [w[0] for w in want] and list(got[1][1, :got[2][1]]) == [w[1] for w in want]


@pytest.mark.parametrize("variant", [OKAPI, BM25S])
def test_agreement_with_the_existing_routes(engine, variant):
    c = _corpus(variant)
    idx = c["idx"]
    engine.set_bm25(idx)
    rng = np.random.default_rng(61)
    dir_id = rng.integers(0, 5, N).astype(np.int16)
    dir_id[:300] = 5                                                       # a small class
    engine.set_doc_meta(N, None, dir_id)
    try:
        csr = _csr(idx, c["queries"])
        for k in (10, 192):
            plain = engine.bm25_topk(*csr, k)
            got = engine.bm25_topk_rows(*csr, k, [np.arange(N)], list_of=np.zeros(NQ, np.int32))
            for a, b in zip(plain, got):
                assert np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))
            col = (np.arange(NQ) % 6).astype(np.int16)
            want = engine.bm25_topk(*csr, k, filter_dir=col)
            lists = [np.flatnonzero(dir_id == cl) for cl in range(6)]
            got = engine.bm25_topk_rows(*csr, k, lists, list_of=col.astype(np.int32))
            for a, b in zip(want, got):
                assert np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))
    finally:
        engine.set_doc_meta(N, None, None)


def test_slots_streams_and_device_outputs(engine):
    import torch
    c, c2 = _corpus(OKAPI), _corpus(BM25S)
    idx, S = c["idx"], c["S"]
    rng = np.random.default_rng(71)
    engine.set_bm25(idx, slot=0)
    other = engine.alloc_bm25_slot()
    try:
        engine.set_bm25(c2["idx"], slot=other)
        lists = [_pick(rng, N, L) for L in (400, 3000, 2048, 0, 2049, 12000)]
        B, k = len(lists), 50
        csr = _csr(idx, c["queries"][:B])
        csr2 = _csr(c2["idx"], c2["queries"][:B])
        _check(engine.bm25_topk_rows(*csr2, k, lists, slot=other), lambda b: c2["S"][b], lists, None, k, B, "other slot")
        host = engine.bm25_topk_rows(*csr, k, lists, slot=0)
        _check(host, lambda b: S[b], lists, None, k, B, "first slot again")
        # host results == device outputs on a non-default stream
        dev = torch.device("cuda", 0)
        s2 = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()
        out = engine.bm25_topk_rows(*csr, k, lists, device_out=True, stream=s2, slot=0)
        engine.sync(s2)
        for a, b in zip(host, out):
            assert np.array_equal(np.asarray(a).view(np.uint8), b.cpu().numpy().view(np.uint8))
        # a device-output bm25_topk followed by a rows call on the same stream: both right after one sync
        plain_host = engine.bm25_topk(*csr, k, slot=0)
        plain = engine.bm25_topk(*csr, k, device_out=True, stream=s2, slot=0)
        rows = engine.bm25_topk_rows(*csr, k, lists, device_out=True, stream=s2, slot=0)
        engine.sync(s2)
        for a, b in zip(plain_host, plain):
            assert np.array_equal(np.asarray(a).view(np.uint8), b.cpu().numpy().view(np.uint8))
        for a, b in zip(host, rows):
            assert np.array_equal(np.asarray(a).view(np.uint8), b.cpu().numpy().view(np.uint8))
    finally:
        engine.free_bm25_slot(other)


def test_errors(engine):
    """Status codes of the entry with the outputs untouched: ERH_ERR_INVALID, ERH_ERR_UNSUPPORTED, ERH_ERR_STATE.  (ERH_ERR_NOMEM needs an
    allocation the device refuses; the work-space option is bounded so that no call can ask for one, as on the dense entry.)"""
    c = _corpus(OKAPI)
    idx = c["idx"]
    engine.set_bm25(idx)
    qi, qt = _csr(idx, c["queries"][:2])
    st = _stats(engine)

    def raw(rows, ptr, lo, k=3, qi_=qi, qt_=qt, eng=engine):
        """The C entry with arbitrary tables; outputs pre-filled so that 'untouched' can be seen."""
        rows, ptr, lo = np.asarray(rows, np.int32), np.asarray(ptr, np.int64), np.asarray(lo, np.int32)
        qi_, qt_ = np.ascontiguousarray(qi_, np.int32), np.ascontiguousarray(qt_, np.int32)
        ids = np.full((2, max(k, 1)), 77, np.int32)
        sc = np.full((2, max(k, 1)), 7.5, np.float64)
        ln = np.full(2, 77, np.int32)
        rc = eng._lib.erh_bm25_topk_rows(eng._h, qi_.ctypes.data, qt_.ctypes.data, 2, k, len(ptr) - 1, ptr.ctypes.data, rows.ctypes.data,
                                         lo.ctypes.data, ids.ctypes.data, sc.ctypes.data, ln.ctypes.data, 0, 0)
        return rc, bool(np.all(ids == 77) and np.all(sc == 7.5) and np.all(ln == 77))

    good = ([1, 5, 9, 2, 3], [0, 3, 5], [0, 1])
    assert raw(*good)[0] == _lib.ERH_OK
    for rows, ptr, lo, who in (([9, 5, 1, 2, 3], [0, 3, 5], [0, 1], "descending"),
                               ([1, 5, 5, 2, 3], [0, 3, 5], [0, 1], "duplicate"),
                               ([1, 5, N, 2, 3], [0, 3, 5], [0, 1], "row == N"),
                               ([-1, 5, 9, 2, 3], [0, 3, 5], [0, 1], "negative row"),
                               ([1, 5, 9, 2, 3], [0, 4, 3], [0, 1], "list_ptr not monotone"),
                               ([1, 5, 9, 2, 3], [0, 3, 5], [0, 2], "list_of == n_lists"),
                               ([1, 5, 9, 2, 3], [0, 3, 5], [-2, 1], "list_of < -1")):
        rc, untouched = raw(rows, ptr, lo)
        assert rc == _lib.ERH_ERR_INVALID and untouched, who
    bad_tok = qt.copy()
    bad_tok[0] = idx.n_vocab
    for qi_, qt_, who in ((qi, bad_tok, "term id == V"), (np.array([0, 5, 3], np.int32), qt, "q_indptr decreases"),
                          (np.array([1, 3, 5], np.int32), qt, "q_indptr[0] != 0")):
        rc, untouched = raw(*good, qi_=qi_, qt_=qt_)
        assert rc == _lib.ERH_ERR_INVALID and untouched, who
    for k in (0, 1025):
        rc, untouched = raw(*good, k=k)
        assert rc == _lib.ERH_ERR_UNSUPPORTED and untouched, k
    assert _moved(engine, st)[0] == {"bm25_rows_calls": 1, "bm25_rows_short_launches": 1, "bm25_rows_long_launches": 0}    # nothing refused was counted
    with pytest.raises(_lib.ErhError, match="status -1"):
        engine.bm25_topk_rows(qi, qt, 3, [np.array([4, 4])] * 2)
    with pytest.raises(_lib.ErhError, match="status -5"):
        engine.bm25_topk_rows(qi, qt, 1025, [np.array([1, 2])] * 2)
    fresh = RetrievalEngine(0)
    try:
        rc, untouched = raw(*good, eng=fresh)                                # no index in the slot
        assert rc == _lib.ERH_ERR_STATE and untouched
    finally:
        fresh.close()


def test_live_bytes_return_after_both_shapes():
    import gc
    c = _corpus(BM25S)
    gc.collect()
    base = live_device_bytes()
    eng = RetrievalEngine(0)
    try:
        eng.set_bm25(c["idx"])
        rng = np.random.default_rng(1)
        lists = [_pick(rng, N, 100), _pick(rng, N, 3000)]
        got = eng.bm25_topk_rows(*_csr(c["idx"], c["queries"][:2]), 10, lists)
        _check(got, lambda b: c["S"][b], lists, None, 10, 2, "fresh handle")
        assert eng.stat("bm25_rows_short_launches") == 1 and eng.stat("bm25_rows_long_launches") == 1
        assert live_device_bytes() - base > 0
    finally:
        eng.close()
    assert live_device_bytes() - base == 0


# ---- retrievers and hybrid on the 103 reference questions ----------------------------------------------------------------------------
@pytest.mark.parametrize("bm25_type", [0, 1])
def test_retrievers_with_rows(bm25_type):
    """BM25Retriever.retrieve_batch(rows=) with and without filter_dict, score_nodes, and HybridRetriever.retrieve_batch(rows=, sparse_rows=)
    of retrieval types 2 and 3 against the oracle composition -- masked BM25 walk, masked dense_exact_topk, reciprocal_rank_fusion -- and
    against the same call made one query at a time."""
    import zlib
    from conftest import WhitespaceTokenizer
    from test_reference_fixtures import DIRS, _fixture, synthetic_text_corpus
    from easyrag_amd.retrievers import BM25Retriever, HipVectorStore, HybridRetriever, QdrantRetriever
    from easyrag_amd.schema import TextNode
    from oracle import dense_exact_topk, reciprocal_rank_fusion, to_f16_unit
    from oracle.retrievers import Item, tokenize_and_remove_stopwords

    class Embedder:
        def get_query_embedding(self, text, d=256):
            v = np.random.default_rng(zlib.crc32(text.encode())).standard_normal(d).astype(np.float32)
            return (v / np.linalg.norm(v)).tolist()

    fx = _fixture()
    texts, dirs = synthetic_text_corpus(fx, n_docs=5000)
    order = np.argsort(np.array([DIRS.index(d) for d in dirs]), kind="stable")
    texts, dirs = [texts[i] for i in order], [dirs[i] for i in order]
    texts[40] = texts[11]
    nodes = [TextNode(text=t, metadata={"dir": d}, id_=f"n{i}") for i, (t, d) in enumerate(zip(texts, dirs))]
    emb, tok, stop = Embedder(), WhitespaceTokenizer(), {""}
    vecs = np.asarray([emb.get_query_embedding(f"doc{i}:" + t) for i, t in enumerate(texts)], np.float32)
    sparse = BM25Retriever.from_defaults(nodes=nodes, tokenizer=tok, similarity_top_k=192, stopwords=stop, bm25_type=bm25_type)
    eng = sparse.engine
    try:
        store = HipVectorStore(nodes, vecs, engine=eng)
        dense = QdrantRetriever(store, emb, similarity_top_k=288)
        queries = [" ".join(q["tokens"]) for q in fx["queries"]]
        B = len(queries)
        docs = [tokenize_and_remove_stopwords(tok, t, stop) for t in texts]
        ora = BM25Okapi(docs, 1.5, 0.75, 0.25) if bm25_type == 0 else BM25SLucene(1.5, 0.75).index(docs)
        S = [ora.get_scores(q["tokens"]) for q in fx["queries"]]
        x16, dir_arr = to_f16_unit(vecs), np.array(dirs)
        n = len(nodes)
        cid = {}
        cid = [cid.setdefault(t, i) for i, t in enumerate(texts)]
        rng = np.random.default_rng(9)
        own = [q["dir"] for q in fx["queries"]]

        def pairs(lst):
            return [(g.node.node_id, g.score) for g in lst]

        def mask_of(rows, fd=None):
            m = np.ones(n, bool)
            if rows is not None:
                m = np.zeros(n, bool)
                m[np.asarray(rows, np.int64)] = True
            if fd:
                m &= dir_arr == fd["dir"]
            return m

        def want_sparse(b, rows, fd=None, k=192):
            return bm25_filter(S[b], k, None if rows is None and not fd else mask_of(rows, fd))

        def want_dense(query, rows, k=288):
            q16 = to_f16_unit(np.asarray(emb.get_query_embedding(query), np.float32))
            return dense_exact_topk(x16, q16, k, None if rows is None else mask_of(rows))

        def named(lst):
            return [(nodes[i].node_id, s) for i, s in lst]

        # BM25Retriever: per-query rows of both shapes, None entries, shared lists, rows + filter_dict
        rows = [_pick(rng, n, int(L)) for L in rng.integers(1, 900, B)]
        rows[1], rows[4] = None, None
        rows[3] = rows[2]
        rows[5] = _pick(rng, n, 2600)
        eng.reset_stats()
        got = sparse.retrieve_batch(queries, rows=rows)
        assert eng.stat("bm25_rows_calls") == 1 and eng.stat("bm25_rows_short_launches") == 1 and eng.stat("bm25_rows_long_launches") == 1
        assert eng.stat("bm25_calls") == 1
        for b in range(B):
            assert pairs(got[b]) == named(want_sparse(b, rows[b])), b
        fds = [{"dir": d} if b % 2 == 0 else None for b, d in enumerate(own)]
        got = sparse.retrieve_batch(queries, filter_dicts=fds, rows=rows)
        for b in range(B):
            assert pairs(got[b]) == named(want_sparse(b, rows[b], fds[b])), b
        one = _pick(rng, n, 300)
        got = sparse.retrieve_batch(queries[:3], rows=one)
        for b in range(3):
            assert pairs(got[b]) == named(want_sparse(b, one)), b
        # score_nodes: the given nodes ranked by the corpus index, positives only; more than one list's worth too
        for cnt in (192, 2500):
            given = _pick(rng, n, cnt)
            got = sparse.score_nodes(queries[0], [nodes[int(i)] for i in given[:5]] + [int(i) for i in given[5:]])
            assert pairs(got) == named(want_sparse(0, given, k=cnt)), cnt
        assert pairs(sparse.score_nodes(queries[0], given, top_k=7)) == pairs(got)[:7]

        # hybrid, retrieval type 2: sparse_rows goes through, rows (the dense route's) does not matter
        hy2 = HybridRetriever(dense, sparse, retrieval_type=2, topk=10)
        got = hy2.retrieve_batch(queries[:8], sparse_rows=rows[:8], rows=[one] * 8)
        for b in range(8):
            assert pairs(got[b]) == named(want_sparse(b, rows[b])), b
        # retrieval type 3: both routes held to lists -- the same object on both, or a list of its own each
        hy = HybridRetriever(dense, sparse, retrieval_type=3, topk=10)
        both = [r if r is not None else one for r in rows]
        drows = [_pick(rng, n, int(L)) for L in rng.integers(1, 900, B)]

        def want_hy(b, srows, dr, fd=None):
            sp = want_sparse(b, srows, fd)
            did, dsc = want_dense(queries[b], dr)
            fused = reciprocal_rank_fusion([[Item(i, cid[i], s) for i, s in sp],
                                            [Item(int(i), cid[int(i)], float(s)) for i, s in zip(did, dsc)]], K=60, topk=10)
            return [(nodes[w.idx].node_id, w.score) for w in fused]

        eng.reset_stats()
        batch = hy.retrieve_batch(queries, rows=both, sparse_rows=both)
        assert (eng.stat("hybrid_calls"), eng.stat("dense_calls"), eng.stat("bm25_calls"), eng.stat("bm25_rows_calls"), eng.stat("dense_rows_calls")) \
            == (0, 0, 0, 1, 1)
        for b in range(B):
            assert pairs(batch[b]) == want_hy(b, both[b], both[b]), b
        batch2 = hy.retrieve_batch(queries, filter_dicts=fds, rows=drows, sparse_rows=both)
        for b in range(B):
            assert pairs(batch2[b]) == want_hy(b, both[b], drows[b], fds[b]), b
        for b in (0, 5, 17):                                                # the same call, one query at a time
            assert pairs(hy.retrieve_batch([queries[b]], rows=[both[b]], sparse_rows=[both[b]])[0]) == pairs(batch[b]), b
            assert pairs(hy2.retrieve_batch([queries[b]], sparse_rows=[rows[b]])[0]) == named(want_sparse(b, rows[b])), b
        # a mixture: some queries without sparse rows -- the routes on their own + RRF
        got = hy.retrieve_batch(queries[:6], rows=both[:6], sparse_rows=rows[:6])
        for b in range(6):
            assert pairs(got[b]) == want_hy(b, rows[b], both[b]), b
    finally:
        sparse.close()
        eng.close()
