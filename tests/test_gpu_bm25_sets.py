"""GPU parity, sparse route with a SET of allowed classes per query (erh_bm25_topk_sets, csrc/bm25_sets.hip): query b ranks the documents whose
class is in its set.  Ids AND fp64 score bits must equal the oracle's masked walk, `bm25_filter(get_scores(q), k, keep_mask=np.isin(dir_id,
set))`, on both variants, and the existing entries where they answer the same question.

The oracle's ranking of a set is computed from ONE get_scores vector per (index, query): bm25_filter walks that vector in canonical order, stops
at the first score <= 0 and keeps the masked documents; `_rank` does the same on the allowed documents alone and is held against bm25_filter
literally inside the sweep, so that a sweep over many sets does not walk the corpus in Python per case."""
import numpy as np
import pytest

from conftest import make_text_corpus
from easyrag_amd import _lib
from easyrag_amd.engine import RetrievalEngine, live_device_bytes, queries_to_csr
from easyrag_amd.index import BM25S, OKAPI, build_bm25_index
from oracle import BM25Okapi, BM25SLucene, bm25_filter

pytestmark = pytest.mark.gpu

KS = (1, 10, 192, 1024)
N, VOCAB, NQ = 6000, 2000, 12
SIZES = (2000, 1900, 1500, 400, 150, 45, 5)        # seven classes of very unequal size
CLASS_IDS = (0, 1, 2, 3, 4, 5, 7)                  # class 6 lies inside the class table and no document carries it; 9 lies beyond it
STATS = ("bm25_calls", "bm25_sets_calls", "bm25_sets_subqueries", "bm25_sets_merge_launches")


def _bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


def _oracle_for(variant, docs):
    return BM25Okapi(docs, k1=1.5, b=0.75, epsilon=0.25) if variant == OKAPI else BM25SLucene(k1=1.5, b=0.75).index(docs)


def _scores(ora, q, n):
    if len(q) == 0:
        return np.zeros(n, np.float64)
    return np.asarray(ora.get_scores(list(q))).astype(np.float64)


def _rank(scores, rows, k):
    """The documents of `rows` (ascending) with a score > 0 under (score desc, id asc), the first k."""
    rows = np.asarray(rows, np.int64)
    s = scores[rows]
    rows, s = rows[s > 0], s[s > 0]
    order = np.lexsort((rows, -s))[:k]
    return rows[order], s[order]


def _allowed(dir_id, st):
    return np.arange(dir_id.shape[0]) if st is None else np.flatnonzero(np.isin(dir_id, np.asarray(list(st), np.int64)))


def _check(got, S_of, dir_id, sets, k, who=""):
    ids, sc, ln = (a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a) for a in got)
    B = len(sets)
    assert ids.shape == (B, k) and sc.shape == (B, k) and ln.shape == (B,)
    for b in range(B):
        oid, osc = _rank(S_of(b), _allowed(dir_id, sets[b]), k)
        assert ln[b] == len(oid), (who, b, int(ln[b]), len(oid))
        assert np.array_equal(ids[b, :ln[b]], oid), (who, b)
        assert np.array_equal(_bits(sc[b, :ln[b]]), _bits(osc)), (who, b)
        assert np.all(ids[b, ln[b]:] == -1) and np.all(sc[b, ln[b]:] == 0.0), (who, b)


def _same(a, b):
    for x, y in zip(a, b):
        x, y = (v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v) for v in (x, y))
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))


def _stats(engine):
    return {n: engine.stat(n) for n in STATS}


def _moved(engine, before):
    after = _stats(engine)
    return {n: after[n] - before[n] for n in after}, after


def _csr(idx, queries):
    return queries_to_csr([idx.tokens_to_ids(q) for q in queries])


def _token_docs(n, vocab, seed):
    return [[int(w[1:]) for w in d.split(" ")] for d in make_text_corpus(n, vocab, seed)]


_CORPORA = {}


def _corpus(variant):
    """Index, oracle, twelve queries and their score vectors [12 x N] (float64), computed once per variant and left unchanged."""
    if variant not in _CORPORA:
        docs = _token_docs(N, VOCAB, seed=2)
        rng = np.random.default_rng(9)
        queries = [[int(t) for t in rng.choice(docs[int(rng.integers(0, N))], size=int(rng.integers(2, 9)))] for _ in range(NQ)]
        ora = _oracle_for(variant, docs)
        S = np.stack([_scores(ora, q, N) for q in queries])
        _CORPORA[variant] = dict(docs=docs, ora=ora, idx=build_bm25_index(docs, variant), queries=queries, S=S)
    return _CORPORA[variant]


def _layout(which):
    blocks = np.repeat(np.asarray(CLASS_IDS, np.int16), SIZES)
    assert blocks.shape[0] == N
    if which == "blocks":
        return blocks
    out = np.asarray(CLASS_IDS, np.int16)[np.arange(N) % 7]              # interleaved: every tile holds every class
    return out


@pytest.fixture
def meta(engine):
    """Class columns are set through this and cleared afterwards, so that no test leaves its column to the next one."""
    def put(dir_id):
        engine.set_doc_meta(int(dir_id.shape[0]), None, dir_id)
    yield put
    engine.set_doc_meta(N, None, None)


@pytest.mark.parametrize("layout", ["blocks", "interleaved"])
@pytest.mark.parametrize("variant", [OKAPI, BM25S])
def test_oracle_sweep(engine, meta, variant, layout):
    c = _corpus(variant)
    idx, S = c["idx"], c["S"]
    engine.set_bm25(idx)
    dir_id = _layout(layout)
    meta(dir_id)
    rng = np.random.default_rng(17 + variant)
    B = 48
    sets = [None, [], [32767], [9], [6], [6, 9, 32767], list(CLASS_IDS), [7], [0, 7], [5, 7, 6]]
    while len(sets) < B:
        m = int(rng.integers(0, 8))
        sets.append([int(x) for x in rng.choice(np.asarray(CLASS_IDS + (6, 9)), size=m, replace=False)] if m else [])
    qs = [c["queries"][b % NQ] for b in range(B)]
    carried = set(CLASS_IDS)
    n_sub = sum(1 if s is None else len(carried & set(s)) for s in sets)
    st = _stats(engine)
    for k in KS:
        got = engine.bm25_topk_sets(*_csr(idx, qs), k, sets)
        mv, st = _moved(engine, st)
        assert mv == {"bm25_calls": 1, "bm25_sets_calls": 1, "bm25_sets_subqueries": n_sub, "bm25_sets_merge_launches": 1}, mv
        _check(got, lambda b: S[b % NQ], dir_id, sets, k, ("sweep", layout, k))
        assert list(np.asarray(got[2])[1:6]) == [0] * 5
    # the helper against the literal oracle walk
    for b in (0, 6, 8, 20, 33):
        want = bm25_filter(c["ora"].get_scores(qs[b]), 192, None if sets[b] is None else np.isin(dir_id, np.asarray(sets[b], np.int64)))
        oid, osc = _rank(S[b % NQ], _allowed(dir_id, sets[b]), 192)
        assert [w[0] for w in want] == list(oid) and np.array_equal(_bits([w[1] for w in want]), _bits(osc)), b


@pytest.mark.parametrize("variant", [OKAPI, BM25S])
def test_full_lists_at_the_merge_capacity(engine, meta, variant):
    """Token 0 sits in every document: every row is positive, every sub-list of k = 1024 is full, and what the truncation after each merge
    step drops decides the answer."""
    n = 4500
    docs = [[0] + d for d in _token_docs(n, 300, seed=4)]
    ora = _oracle_for(variant, docs)
    idx = build_bm25_index(docs, variant)
    engine.set_bm25(idx)
    dir_id = (np.arange(n) % 3).astype(np.int16)
    meta(dir_id)
    queries = [[0], [0, 5], [0, 17, 3], [0, 0, 9]]
    sets = [[0, 1], [1, 2, 0], [2, 0], [0, 1, 2]]
    Sq = [_scores(ora, q, n) for q in queries]
    for k in (1024, 1000):
        got = engine.bm25_topk_sets(*_csr(idx, queries), k, sets)
        assert np.all(np.asarray(got[2]) == k)
        _check(got, lambda b: Sq[b], dir_id, sets, k, ("capacity", k))


@pytest.mark.parametrize("variant", [OKAPI, BM25S])
def test_deep_chain_of_short_lists(engine, meta, variant):
    """40 classes of 5 ... 50 documents, sets of 1 ... 40 classes, k = 192; a rare token leaves classes inside a set with empty sub-lists."""
    rng = np.random.default_rng(12)
    sizes = rng.integers(5, 51, 40)
    n = int(sizes.sum())
    docs = _token_docs(n, 400, seed=6)
    dir_id = rng.permutation(np.repeat(np.arange(40, dtype=np.int16), sizes))
    ora = _oracle_for(variant, docs)
    idx = build_bm25_index(docs, variant)
    engine.set_bm25(idx)
    meta(dir_id)
    df = np.bincount(np.concatenate([np.unique(d) for d in docs]), minlength=400)
    rare = int(np.flatnonzero((df >= 3) & (df <= 8))[0])
    queries = [[rare], [0, 1], [rare, rare], [2, 7, rare], [3]] * 8
    sets = [[int(x) for x in rng.permutation(40)[:m]] for m in range(1, 41)]
    sets[39] = list(range(40))
    Sq = [_scores(ora, q, n) for q in queries[:5]]
    with_rare = set(int(x) for x in dir_id[Sq[0] > 0])
    assert any(x not in with_rare for x in range(min(with_rare) + 1, max(with_rare))), "no interior class without the rare token"
    got = engine.bm25_topk_sets(*_csr(idx, queries), 192, sets)
    _check(got, lambda b: Sq[b % 5], dir_id, sets, 192, "deep chain")
    assert np.asarray(got[2]).max() == 192


@pytest.mark.parametrize("variant", [OKAPI, BM25S])
def test_ties_across_classes_come_out_in_id_order(engine, meta, variant):
    n = 900
    docs = _token_docs(n, 200, seed=8)
    planted = list(range(100, 900, 20))                                      # 40 documents with one token list, over three interleaved classes
    for i in planted:
        docs[i] = [150, 151, 151, 152, 7]
    ora = _oracle_for(variant, docs)
    idx = build_bm25_index(docs, variant)
    engine.set_bm25(idx)
    dir_id = (np.arange(n) % 3).astype(np.int16)
    assert len({int(dir_id[i]) for i in planted}) == 3
    meta(dir_id)
    queries = [[150, 151], [151, 152, 150], [150]]
    sets = [[0, 1, 2], [2, 0], [1, 2, 0]]
    Sq = [_scores(ora, q, n) for q in queries]
    for k in (10, 30, 192):
        got = engine.bm25_topk_sets(*_csr(idx, queries), k, sets)
        _check(got, lambda b: Sq[b], dir_id, sets, k, ("ties", k))
    ids = np.asarray(got[0])[0, :40]
    assert list(ids) == planted                                              # one score, three sub-lists: ascending ids across them


@pytest.mark.parametrize("variant", [OKAPI, BM25S])
def test_degenerate_queries_and_the_mixed_launch(engine, meta, variant):
    """An empty query, an all-out-of-vocabulary query, repeated tokens, and a 45-token query among short ones in a batch of more than 512
    sub-queries: the scan underneath takes whatever launch erh_bm25_topk takes for the same sub-query batch."""
    c = _corpus(variant)
    idx, ora, Q = c["idx"], c["ora"], c["queries"]
    engine.set_bm25(idx)
    dir_id = _layout("blocks")
    meta(dir_id)
    long45 = (Q[0] + Q[1] + Q[2] + Q[3] + Q[4] + Q[5] + Q[6] + Q[7] + Q[8] + Q[9] + Q[10] + Q[11])[:45]
    assert len(long45) == 45
    special = [[], [VOCAB + 5, VOCAB + 6], Q[6] + Q[6], long45, Q[3] + [Q[3][0]]]
    qs = special + [Q[b % NQ] for b in range(275)]
    B = len(qs)
    Ssp = [_scores(ora, [t for t in q if t < VOCAB], N) for q in special]
    assert not np.array_equal(Ssp[2], c["S"][6])                             # (a repeated token counts twice)
    sets = [[0, 1] if b % 2 == 0 else [2, 0] for b in range(B)]
    sets[3] = [1, 0, 2]
    csr = _csr(idx, qs)
    mixed0 = engine.stat("bm25_mixed_launches")
    got = engine.bm25_topk_sets(*csr, 10, sets)
    mixed_sets = engine.stat("bm25_mixed_launches") - mixed0
    _check(got, lambda b: Ssp[b] if b < 5 else c["S"][(b - 5) % NQ], dir_id, sets, 10, "degenerate")
    assert got[2][0] == 0 and got[2][1] == 0
    # the same sub-query batch as a plain class-column call: the same launch decision
    sub_q = [qs[b] for b in range(B) for _ in sets[b]]
    col = np.asarray([cl for b in range(B) for cl in sets[b]], np.int16)
    assert len(sub_q) == 2 * B + 1 > 512
    mixed0 = engine.stat("bm25_mixed_launches")
    engine.bm25_topk(*_csr(idx, sub_q), 10, filter_dir=col)
    assert engine.stat("bm25_mixed_launches") - mixed0 == mixed_sets


@pytest.mark.parametrize("variant", [OKAPI, BM25S])
def test_agreement_with_the_existing_entries(engine, meta, variant):
    c = _corpus(variant)
    idx = c["idx"]
    engine.set_bm25(idx)
    dir_id = _layout("interleaved")
    meta(dir_id)
    csr = _csr(idx, c["queries"])
    for k in (10, 192):
        col = np.asarray([CLASS_IDS[b % 7] for b in range(NQ)], np.int16)
        _same(engine.bm25_topk(*csr, k, filter_dir=col), engine.bm25_topk_sets(*csr, k, [[int(x)] for x in col]))
        plain = engine.bm25_topk(*csr, k)
        _same(plain, engine.bm25_topk_sets(*csr, k, [None] * NQ))
        _same(plain, engine.bm25_topk_sets(*csr, k, [list(CLASS_IDS)] * NQ))
        # a set == the numpy canonical merge of the single-class answers
        sets = [[0, 3, 5], [1, 2], [7, 4, 0, 1]] * 4
        got = engine.bm25_topk_sets(*csr, k, sets)
        single = {cl: engine.bm25_topk(*csr, k, filter_dir=np.full(NQ, cl, np.int16)) for cl in CLASS_IDS}
        for b in range(NQ):
            ids = np.concatenate([single[cl][0][b, :single[cl][2][b]] for cl in sets[b]])
            sc = np.concatenate([single[cl][1][b, :single[cl][2][b]] for cl in sets[b]])
            order = np.lexsort((ids, -sc))[:k]
            assert got[2][b] == len(order) and np.array_equal(got[0][b, :len(order)], ids[order]), (k, b)
            assert np.array_equal(_bits(got[1][b, :len(order)]), _bits(sc[order])), (k, b)


def test_chunk_boundary(engine, meta):
    """2800 queries x 3 classes = 8400 sub-queries: two chunks (8192 + 208), query 2730's sub-queries on both sides; one merge."""
    n, B, k = 3000, 2800, 10
    docs = _token_docs(n, 500, seed=3)
    ora = _oracle_for(BM25S, docs)
    idx = build_bm25_index(docs, BM25S)
    engine.set_bm25(idx)
    dir_id = (np.arange(n) % 4).astype(np.int16)
    meta(dir_id)
    base = [[1, 9], [4], [30, 2, 8], [17, 5], [3, 3, 40], [11], [6, 21]]
    Sq = [_scores(ora, q, n) for q in base]
    qs = [base[b % 7] for b in range(B)]
    sets = [[(b + j) % 4 for j in range(3)] for b in range(B)]
    assert 8192 % 3 != 0
    st = _stats(engine)
    got = engine.bm25_topk_sets(*_csr(idx, qs), k, sets)
    mv, _ = _moved(engine, st)
    assert mv == {"bm25_calls": 1, "bm25_sets_calls": 1, "bm25_sets_subqueries": 8400, "bm25_sets_merge_launches": 1}, mv
    _check(got, lambda b: Sq[b % 7], dir_id, sets, k, "chunks")


def test_okapi_index_with_negative_idf(engine, meta):
    """rank-bm25's epsilon * average_idf floor is negative when most terms sit in most documents: the index takes the order-keeping scans
    underneath, and a document whose sum is <= 0 is not returned."""
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
    dir_id = rng.integers(0, 4, 3000).astype(np.int16)
    meta(dir_id)
    queries = [[0, 1, 7], [6, 7, 2, 2], [7], [3], [6, 0, 1, 2, 3, 4, 5]]
    sets = [[0, 1], [3, 1, 2], [0, 1, 2, 3], [2, 0], None]
    Sq = [_scores(ora, q, 3000) for q in queries]
    for k in (5, 150):
        got = engine.bm25_topk_sets(*_csr(idx, queries), k, sets)
        _check(got, lambda b: Sq[b], dir_id, sets, k, ("negative idf", k))
    want = bm25_filter(ora.get_scores(queries[1]), 150, np.isin(dir_id, [1, 2, 3]))         # the literal oracle once more
    assert list(got[0][1, :got[2][1]]) == [w[0] for w in want] and list(got[1][1, :got[2][1]]) == [w[1] for w in want]


def test_slots_streams_and_device_outputs(engine, meta):
    import torch
    c, c2 = _corpus(OKAPI), _corpus(BM25S)
    idx, S = c["idx"], c["S"]
    dir_id = _layout("blocks")
    meta(dir_id)
    engine.set_bm25(idx, slot=0)
    other = engine.alloc_bm25_slot()
    try:
        engine.set_bm25(c2["idx"], slot=other)
        sets = [[0, 1], None, [2, 3, 4], [], [7, 0], [1, 5, 6]]
        B, k = len(sets), 50
        csr, csr2 = _csr(idx, c["queries"][:B]), _csr(c2["idx"], c2["queries"][:B])
        host = engine.bm25_topk_sets(*csr, k, sets, slot=0)
        _check(host, lambda b: S[b], dir_id, sets, k, "slot 0")
        _check(engine.bm25_topk_sets(*csr2, k, sets, slot=other), lambda b: c2["S"][b], dir_id, sets, k, "other slot")
        _same(host, engine.bm25_topk_sets(*csr, k, sets, slot=0))           # ... which left slot 0's answers as they were
        # device outputs on a non-default stream, read after one sync
        s2 = torch.cuda.Stream(device=torch.device("cuda", 0))
        torch.cuda.synchronize()
        out = engine.bm25_topk_sets(*csr, k, sets, device_out=True, stream=s2, slot=0)
        engine.sync(s2)
        _same(host, out)
        # a device-output bm25_topk in front on the same stream keeps its results
        plain_host = engine.bm25_topk(*csr, k, slot=0)
        plain = engine.bm25_topk(*csr, k, device_out=True, stream=s2, slot=0)
        out = engine.bm25_topk_sets(*csr, k, sets, device_out=True, stream=s2, slot=0)
        engine.sync(s2)
        _same(plain_host, plain)
        _same(host, out)
    finally:
        engine.free_bm25_slot(other)


def test_status_codes_leave_the_outputs_untouched(engine, meta):
    c = _corpus(OKAPI)
    idx = c["idx"]
    engine.set_bm25(idx)
    meta(_layout("blocks"))
    qi, qt = _csr(idx, c["queries"][:2])
    st = _stats(engine)

    def raw(ptr, cls, k=3, qi_=qi, qt_=qt, eng=engine, null_cls=False):
        ptr, cls = np.asarray(ptr, np.int32), np.asarray(cls, np.int16)
        qi_, qt_ = np.ascontiguousarray(qi_, np.int32), np.ascontiguousarray(qt_, np.int32)
        ids = np.full((2, max(k, 1)), 77, np.int32)
        sc = np.full((2, max(k, 1)), 7.5, np.float64)
        ln = np.full(2, 77, np.int32)
        rc = eng._lib.erh_bm25_topk_sets(eng._h, qi_.ctypes.data, qt_.ctypes.data, 2, k, ptr.ctypes.data, 0 if null_cls else cls.ctypes.data,
                                         ids.ctypes.data, sc.ctypes.data, ln.ctypes.data, 0, 0)
        return rc, bool(np.all(ids == 77) and np.all(sc == 7.5) and np.all(ln == 77))

    good = ([0, 2, 3], [0, 1, 2])
    assert raw(*good) == (_lib.ERH_OK, False)
    for ptr, cls, kw, who in (([0, 3, 2], [0, 1, 2], {}, "set_ptr not monotone"), ([1, 2, 3], [0, 1, 2], {}, "set_ptr[0] != 0"),
                              ([0, 2, 3], [0, -2, 2], {}, "negative class"), ([0, 2, 3], [0, -1, 2], {}, "-1 beside a class"),
                              ([0, 2, 3], [1, 1, 2], {}, "a class twice"), ([0, 2, 3], [0, 1, 2], {"null_cls": True}, "null set_cls")):
        rc, untouched = raw(ptr, cls, **kw)
        assert rc == _lib.ERH_ERR_INVALID and untouched, who
    bad_tok = qt.copy()
    bad_tok[0] = idx.n_vocab
    for qi_, qt_, who in ((qi, bad_tok, "term id == V"), (np.array([0, 5, 3], np.int32), qt, "q_indptr decreases")):
        rc, untouched = raw(*good, qi_=qi_, qt_=qt_)
        assert rc == _lib.ERH_ERR_INVALID and untouched, who
    for k in (0, 1025):
        rc, untouched = raw(*good, k=k)
        assert rc == _lib.ERH_ERR_UNSUPPORTED and untouched, k
    assert _moved(engine, st)[0] == {"bm25_calls": 1, "bm25_sets_calls": 1, "bm25_sets_subqueries": 3, "bm25_sets_merge_launches": 1}
    engine.set_doc_meta(N, None, None)                                       # no class column
    rc, untouched = raw(*good)
    assert rc == _lib.ERH_ERR_STATE and untouched
    assert raw([0, 1, 2], [-1, -1])[0] == _lib.ERH_OK                        # {-1} needs none
    assert raw([0, 0, 0], [], null_cls=True)[0] == _lib.ERH_OK               # nor do empty sets
    engine.set_doc_meta(N - 1, None, _layout("blocks")[:N - 1])              # a column that does not cover the slot's documents
    rc, untouched = raw(*good)
    assert rc == _lib.ERH_ERR_STATE and untouched
    with pytest.raises(_lib.ErhError, match="status -5"):
        engine.bm25_topk_sets(qi, qt, 1025, [None, None])
    fresh = RetrievalEngine(0)
    try:
        rc, untouched = raw(*good, eng=fresh)                                # no index in the slot
        assert rc == _lib.ERH_ERR_STATE and untouched
    finally:
        fresh.close()


def test_live_bytes_return(engine):
    import gc
    c = _corpus(BM25S)
    gc.collect()
    base = live_device_bytes()
    eng = RetrievalEngine(0)
    try:
        eng.set_bm25(c["idx"])
        dir_id = _layout("blocks")
        eng.set_doc_meta(N, None, dir_id)
        sets = [[0, 1, 2], None]
        got = eng.bm25_topk_sets(*_csr(c["idx"], c["queries"][:2]), 10, sets)
        _check(got, lambda b: c["S"][b], dir_id, sets, 10, "fresh handle")
        assert eng.stat("bm25_sets_merge_launches") == 1
        assert live_device_bytes() - base > 0
    finally:
        eng.close()
    assert live_device_bytes() - base == 0


# ---- retrievers and hybrid on the 103 reference questions ----------------------------------------------------------------------------
@pytest.mark.parametrize("bm25_type", [0, 1])
def test_retrievers_with_set_filters(bm25_type):
    """BM25Retriever(filters=MatchAny over two dirs) against the oracle's masked walk, and HybridRetriever with the same filter on both routes
    against the oracle composition -- masked bm25_filter + masked dense_exact_topk -> reciprocal_rank_fusion; without sparse_filters the
    sparse route stays unfiltered, as today."""
    import zlib
    from conftest import WhitespaceTokenizer
    from test_filter_grammar import FieldCondition, Filter, MatchAny, MatchValue
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
        assert B == 103
        docs = [tokenize_and_remove_stopwords(tok, t, stop) for t in texts]
        ora = BM25Okapi(docs, 1.5, 0.75, 0.25) if bm25_type == 0 else BM25SLucene(1.5, 0.75).index(docs)
        S = [ora.get_scores(q["tokens"]) for q in fx["queries"]]
        x16, dir_arr = to_f16_unit(vecs), np.array(dirs)
        cid = {}
        cid = [cid.setdefault(t, i) for i, t in enumerate(texts)]
        two = [DIRS[0], DIRS[1]]
        flt = Filter(must=[FieldCondition(key="dir", match=MatchAny(any=two))])
        mask = np.isin(dir_arr, two)

        def pairs(lst):
            return [(g.node.node_id, g.score) for g in lst]

        def named(lst):
            return [(nodes[i].node_id, s) for i, s in lst]

        # BM25Retriever: the attribute, the argument, and filter_dict AND filters
        sparse.filters = flt
        eng.reset_stats()
        got = sparse.retrieve_batch(queries)
        assert eng.stat("bm25_sets_calls") == 1 and eng.stat("bm25_sets_subqueries") == 2 * B and eng.stat("bm25_calls") == 1
        for b in range(B):
            assert pairs(got[b]) == named(bm25_filter(S[b], 192, mask)), b
        sparse.filters = None
        not3 = Filter(must_not=[FieldCondition(key="dir", match=MatchValue(value=DIRS[3]))])
        got = sparse.retrieve_batch(queries[:20], filters=not3, filter_dicts=[{"dir": DIRS[b % 4]} if b % 3 == 0 else None for b in range(20)])
        for b in range(20):
            m = dir_arr != DIRS[3]
            if b % 3 == 0:
                m = m & (dir_arr == DIRS[b % 4])
            assert pairs(got[b]) == named(bm25_filter(S[b], 192, m)), b

        def want_hy(b, s_mask, d_mask):
            sp = bm25_filter(S[b], 192, s_mask)
            q16 = to_f16_unit(np.asarray(emb.get_query_embedding(queries[b]), np.float32))
            did, dsc = dense_exact_topk(x16, q16, 288, d_mask)
            fused = reciprocal_rank_fusion([[Item(i, cid[i], s) for i, s in sp],
                                            [Item(int(i), cid[int(i)], float(s)) for i, s in zip(did, dsc)]], K=60, topk=10)
            return [(nodes[w.idx].node_id, w.score) for w in fused]

        hy = HybridRetriever(dense, sparse, retrieval_type=3, topk=10)
        eng.reset_stats()
        batch = hy.retrieve_batch(queries, filters=flt, sparse_filters=flt)
        assert (eng.stat("hybrid_calls"), eng.stat("dense_calls"), eng.stat("bm25_calls"), eng.stat("bm25_sets_calls")) == (0, 1, 1, 1)
        for b in range(B):
            assert pairs(batch[b]) == want_hy(b, mask, mask), b
        eng.reset_stats()
        today = hy.retrieve_batch(queries, filters=flt)                      # the sparse route sees the whole corpus, as in the reference
        assert eng.stat("bm25_sets_calls") == 0
        for b in range(B):
            assert pairs(today[b]) == want_hy(b, None, mask), b
    finally:
        sparse.close()
        eng.close()
