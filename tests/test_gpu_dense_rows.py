"""GPU parity, dense route over explicit per-query row lists (erh_dense_topk_rows, csrc/dense_rows.hip): query b ranks the rows of its list
and nothing else.  Every listed row gets the pinned-order fp64 score, so ids AND fp64 score bits must equal the oracle's masked ranking,
`oracle.dense_exact_topk(x16, q16, k, mask)`, on both kernel shapes (lists of at most 2048 rows: one launch; longer: score + select), and the
existing routes where they answer the same question (all rows = unfiltered erh_dense_topk, the rows of a class = the class column).

The oracle's ranking of a list is computed here from ONE `dense_exact_scores` vector per (corpus, query vector) -- `dense_exact_topk` does
exactly that and then masks; `_rank` is held against it literally in test_rank_helper_is_the_oracle -- so that a sweep over many lists of
one corpus does not recompute 60 000 x d products per case."""
import numpy as np
import pytest

from easyrag_amd import _lib, synth
from oracle import dense_exact_topk, to_f16_unit
from oracle.dense import dense_exact_scores

pytestmark = pytest.mark.gpu

KS = (1, 10, 288, 768)
NB = 7                      # distinct query vectors per corpus: query b carries vector b % NB (7 is coprime with the kernels' group of 8)


def _bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


def _rank(scores, rows, k):
    """Canonical top k (score desc, row id asc) of `rows` (ascending) under the oracle's score vector."""
    rows = np.asarray(rows, np.int64)
    s = scores[rows]
    order = np.lexsort((rows, -s))[:k]
    return rows[order], s[order]


def _unit16(n, d, rng):
    out = np.empty((n, d), np.float16)
    for r0 in range(0, n, 8192):
        out[r0:r0 + 8192] = to_f16_unit(rng.standard_normal((min(8192, n - r0), d), dtype=np.float32))
    return out


_CORPORA = {}


def _corpus(d):
    """(x16 [N x d], base query vectors [NB x d], oracle score vectors [NB x N]); N is odd and no multiple of any tile."""
    if d not in _CORPORA:
        rng = np.random.default_rng(1000 + d)
        n = 60037 if d <= 1024 else 52117
        x = _unit16(n, d, rng)
        base = to_f16_unit(x[rng.integers(0, n, NB)].astype(np.float32) + 0.7 * rng.standard_normal((NB, d)).astype(np.float32) / np.sqrt(d))
        S = np.stack([dense_exact_scores(x, base[j]) for j in range(NB)])
        _CORPORA.clear()                                     # one corpus in memory at a time
        _CORPORA[d] = (x, base, S)
    return _CORPORA[d]


def _check(got, S, lists, list_of, k, B, who=""):
    ids, sc, ln = (np.asarray(a.cpu()) if hasattr(a, "cpu") else np.asarray(a) for a in got)
    for b in range(B):
        l = b if list_of is None else int(list_of[b])
        rows = np.zeros(0, np.int64) if l < 0 else lists[l]
        oid, osc = _rank(S[b % NB], rows, k)
        assert ln[b] == min(k, len(rows)) == len(oid), (who, b)
        assert np.array_equal(ids[b, :ln[b]], oid), (who, b)
        assert np.array_equal(_bits(sc[b, :ln[b]]), _bits(osc)), (who, b)
        assert np.all(ids[b, ln[b]:] == -1) and np.all(sc[b, ln[b]:] == 0.0), (who, b)


def _pick(rng, n, length):
    if length >= n:
        return np.arange(n, dtype=np.int64)
    return np.sort(rng.choice(n, size=length, replace=False)).astype(np.int64)


def _moved(engine, before):
    after = {n: engine.stat(n) for n in ("dense_rows_calls", "dense_rows_short_launches", "dense_rows_long_launches")}
    return {n: after[n] - before[n] for n in after}, after


def _stats(engine):
    return {n: engine.stat(n) for n in ("dense_rows_calls", "dense_rows_short_launches", "dense_rows_long_launches")}


def test_rank_helper_is_the_oracle():
    rng = np.random.default_rng(3)
    x = _unit16(3001, 192, rng)
    q = to_f16_unit(rng.standard_normal((2, 192), dtype=np.float32))
    for j, length in ((0, 0), (0, 1), (1, 700), (1, 3001)):
        rows = _pick(rng, 3001, length)
        mask = np.zeros(3001, bool)
        mask[rows] = True
        oid, osc = dense_exact_topk(x, q[j], 50, mask)
        gid, gsc = _rank(dense_exact_scores(x, q[j]), rows, 50)
        assert np.array_equal(oid, gid) and np.array_equal(_bits(osc), _bits(gsc))


@pytest.mark.parametrize("d", [64, 256, 1024, 3584])
def test_parity_sweep(engine, d):
    import torch
    x, base, S = _corpus(d)
    n = x.shape[0]
    rng = np.random.default_rng(d)
    engine.set_dense(x)
    engine.set_doc_meta(n, None, None)
    st = _stats(engine)

    def q_of(B):
        return base[np.arange(B) % NB]

    # every length of the issue, one list per query, both shapes in one call; every k
    for k in KS:
        lens = [0, 1, max(k - 1, 0), k, k + 1, 2047, 2048, 2049, 50000, n, 5, 300, 2500, 0, 1000, 2048, 4097]
        B = len(lens)                                                       # 17
        lists = [_pick(rng, n, L) for L in lens]
        got = engine.dense_topk_rows(q_of(B), k, lists)
        mv, st = _moved(engine, st)
        assert mv == {"dense_rows_calls": 1, "dense_rows_short_launches": 1, "dense_rows_long_launches": 1}, mv
        _check(got, S, lists, None, k, B, ("distinct", k))
        if k == 10:
            # host result == device outputs on a non-default stream == fp32 queries (fp16 values widened: the rounding is the identity)
            dev = torch.device("cuda", 0)
            s2 = torch.cuda.Stream(device=dev)
            qd = torch.from_numpy(q_of(B)).to(dev)
            torch.cuda.synchronize()
            out = engine.dense_topk_rows(qd, k, lists, device_out=True, stream=s2)
            engine.sync(s2)
            for a, b in zip(got, out):
                assert np.array_equal(np.asarray(a).view(np.uint8), b.cpu().numpy().view(np.uint8))
            out32 = engine.dense_topk_rows(q_of(B).astype(np.float32), k, lists)
            for a, b in zip(got, out32):
                assert np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))
            # a check behind rows calls alone: OK, nothing exhaustive
            engine.dense_check()
            assert engine.dense_diag()["exhaustive"] == 0
            mv, st = _moved(engine, st)
            assert mv["dense_rows_calls"] == 2

    # one list shared by all queries: B x length x k, short and long shape
    for B, k, L in ((1, 768, n), (1, 1, 2048), (17, 288, 50000), (17, 10, 2047), (256, 10, n), (256, 768, 2048), (1030, 288, 2049), (1030, 1, 1),
                    (1030, 10, 0)):
        lists = [_pick(rng, n, L)]
        lo = np.zeros(B, np.int32)
        got = engine.dense_topk_rows(q_of(B), k, lists, list_of=lo)
        mv, st = _moved(engine, st)
        short = L <= 2048
        assert mv == {"dense_rows_calls": 1, "dense_rows_short_launches": int(short), "dense_rows_long_launches": int(not short)}, (B, k, L, mv)
        _check(got, S, lists, lo, k, B, ("shared", B, k, L))

    # many queries, distinct lists: short ones, long ones (a work item group of one query), a few lists shared by runs of queries, and -1
    B, k = 1030, 10
    lists = [_pick(rng, n, int(L)) for L in rng.integers(0, 400, B)]
    got = engine.dense_topk_rows(q_of(B), k, lists)
    mv, st = _moved(engine, st)
    assert mv == {"dense_rows_calls": 1, "dense_rows_short_launches": 1, "dense_rows_long_launches": 0}, mv
    _check(got, S, lists, None, k, B, "distinct-1030")
    B, k = 256, 288
    lists = [_pick(rng, n, int(L)) for L in rng.integers(2049, 3000, 40)]
    lo = rng.integers(-1, 40, B).astype(np.int32)
    lo[3] = -1
    got = engine.dense_topk_rows(q_of(B), k, lists, list_of=lo)
    mv, st = _moved(engine, st)
    assert mv["dense_rows_long_launches"] == 1 and mv["dense_rows_short_launches"] == 1, mv     # (-1 entries: the short shape writes the padding)
    _check(got, S, lists, lo, k, B, "grouped-256")


def test_long_shape_runs_in_chunks_when_the_work_space_is_small(engine):
    x, base, S = _corpus(256)
    n = x.shape[0]
    rng = np.random.default_rng(5)
    engine.set_dense(x)
    B, k = 17, 100
    lists = [_pick(rng, n, 20000), _pick(rng, n, 2049)]
    lo = (np.arange(B) % 2).astype(np.int32)
    q = base[np.arange(B) % NB]
    want = engine.dense_topk_rows(q, k, lists, list_of=lo)
    _check(want, S, lists, lo, k, B, "one chunk")
    engine.set_option("dense_rows_ws_mb", 0)                  # the minimum: one list of N rows -- 60037 doubles, two 20000-row spans + ...
    try:
        st = _stats(engine)
        got = engine.dense_topk_rows(q, k, lists, list_of=lo)
        mv, _ = _moved(engine, st)
        assert mv["dense_rows_long_launches"] >= 4, mv
    finally:
        engine.set_option("dense_rows_ws_mb", 256)
    for a, b in zip(want, got):
        assert np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))


@pytest.mark.parametrize("d", [64, 256, 1024])
def test_normalize_q_on_the_device(engine, d):
    """Queries of +-0.5 entries: the device's fp32 normalisation is exact for them (sum of squares d / 4, a power of four), so the fp16
    query it scores is +-1 / sqrt(d) exactly and the oracle applies bit for bit; fp32 and fp16 inputs."""
    x, base, S = _corpus(d)
    n = x.shape[0]
    rng = np.random.default_rng(17 + d)
    engine.set_dense(x)
    B, k = 5, 50
    sign = np.where(rng.random((B, d)) < 0.5, -1.0, 1.0)
    want_q = (sign / np.sqrt(d)).astype(np.float16)
    lists = [_pick(rng, n, L) for L in (300, 2048, 2049, 0, 9000)]
    for q in ((0.5 * sign).astype(np.float32), (0.5 * sign).astype(np.float16)):
        ids, sc, ln = engine.dense_topk_rows(q, k, lists, normalize_q=True)
        for b in range(B):
            mask = np.zeros(n, bool)
            mask[lists[b]] = True
            oid, osc = dense_exact_topk(x, want_q[b], k, mask)
            assert ln[b] == len(oid) and np.array_equal(ids[b, :ln[b]], oid) and np.array_equal(_bits(sc[b, :ln[b]]), _bits(osc)), (d, b)


def test_normalize_q_equals_the_scan_route(engine):
    """d = 3584 (no exact normalisation exists): the rows entry over all rows and erh_dense_topk prepare the query with the same kernel."""
    rng = np.random.default_rng(23)
    n, d, k = 5003, 3584, 100
    x = _unit16(n, d, rng)
    q32 = (rng.standard_normal((6, d)) * 0.3).astype(np.float32)
    engine.set_dense(x)
    want = engine.dense_topk(q32, k, normalize_q=True)
    got = engine.dense_topk_rows(q32, k, [np.arange(n)], list_of=np.zeros(6, np.int32), normalize_q=True)
    for a, b in zip(want, got):
        assert np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))


def test_ties_rank_by_ascending_id(engine):
    """Exact duplicate rows in clusters of 3 and of 40 that straddle the cut: canonical order, in which the oracle alone is deterministic."""
    rng = np.random.default_rng(41)
    n, d = 30011, 256
    x = _unit16(n, d, rng)
    hot = x[5].copy()
    c40 = np.sort(np.concatenate([[5], rng.choice(np.arange(6, n), size=39, replace=False)]))      # 40 copies, row 5 itself included
    x[c40] = hot
    near = to_f16_unit(hot.astype(np.float32) + 0.05 * rng.standard_normal(d).astype(np.float32) / np.sqrt(d))
    c3 = np.sort(rng.choice(np.setdiff1d(np.arange(n), c40), size=3, replace=False))
    x[c3] = near
    engine.set_dense(x)
    q = np.stack([hot, hot, near])
    S3 = np.stack([dense_exact_scores(x, v) for v in q])
    everything = np.arange(n)
    short = np.sort(np.concatenate([c40, c3, rng.choice(n, size=1500, replace=False)]))
    short = np.unique(short)
    for lists, who in (([everything], "long"), ([short], "short")):
        for k in (20, 41, 42):                                              # cuts inside the 40-cluster and inside the 3-cluster
            ids, sc, ln = engine.dense_topk_rows(q, k, lists, list_of=np.zeros(3, np.int32))
            for b in range(3):
                oid, osc = _rank(S3[b], lists[0], k)
                assert np.array_equal(ids[b, :ln[b]], oid) and np.array_equal(_bits(sc[b, :ln[b]]), _bits(osc)), (who, k, b)
            tied = ids[0][sc[0] == sc[0, 0]]
            assert len(tied) == min(k, 40) and np.all(np.diff(tied) > 0) and np.array_equal(tied, c40[:len(tied)])
    mask = np.zeros(n, bool)
    mask[short] = True
    oid, osc = dense_exact_topk(x, q[2], 41, mask)                          # the literal oracle once more
    ids, sc, ln = engine.dense_topk_rows(q[2:3], 41, [short])
    assert np.array_equal(ids[0], oid) and np.array_equal(_bits(sc[0]), _bits(osc))


@pytest.mark.parametrize("blocks", [0, 1])
def test_consistency_with_the_existing_routes(engine, blocks):
    rng = np.random.default_rng(61)
    sizes, d, k = [9000, 300, 7000, 5000, 41], 256, 100
    dir_id = np.repeat(np.arange(len(sizes)), sizes).astype(np.int16)
    tail = dir_id[sizes[0]:].copy()                                         # class 0 stays one contiguous run (a block), the rest is shuffled
    rng.shuffle(tail)
    dir_id[sizes[0]:] = tail
    n = dir_id.shape[0]
    x = _unit16(n, d, rng)
    q16 = to_f16_unit(rng.standard_normal((10, d), dtype=np.float32))
    engine.set_dense(x)
    engine.set_doc_meta(n, None, dir_id)
    engine.set_option("dense_dir_blocks", blocks)
    try:
        plain = engine.dense_topk(q16, k)
        got = engine.dense_topk_rows(q16, k, [np.arange(n)], list_of=np.zeros(10, np.int32))
        for a, b in zip(plain, got):
            assert np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))
        col = (np.arange(10) % len(sizes)).astype(np.int16)
        want = engine.dense_topk(q16, k, filter_dir=col)
        lists = [np.flatnonzero(dir_id == c) for c in range(len(sizes))]
        got = engine.dense_topk_rows(q16, k, lists, list_of=col.astype(np.int32))
        for a, b in zip(want, got):
            assert np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))
    finally:
        engine.set_option("dense_dir_blocks", 1)


def test_rows_call_between_a_dense_call_and_its_check(engine):
    """A device-output erh_dense_topk whose queries need the exhaustive path at the check (17000 copies of the query: beyond the candidate
    budget), a rows call in between: both results right; the rows call counts no exhaustive query of its own."""
    import torch
    rng = np.random.default_rng(53)
    n, d, k = 40000, 256, 100
    x = _unit16(n, d, rng)
    hot = to_f16_unit(rng.standard_normal((1, d), dtype=np.float32))[0]
    copies = np.sort(rng.choice(22000, size=17000, replace=False))
    x[copies] = hot
    engine.set_dense(x)
    engine.set_doc_meta(n, None, None)
    q16 = np.stack([hot, to_f16_unit(rng.standard_normal((1, d), dtype=np.float32))[0], hot])
    lists = [_pick(rng, n, 3000), _pick(rng, n, 500), copies]
    qd = torch.from_numpy(q16).cuda()
    engine.reset_stats()
    dev = engine.dense_topk(qd, k, device_out=True)
    rows_dev = engine.dense_topk_rows(qd[[1, 2, 0]], k, lists, device_out=True)
    rows_host = engine.dense_topk_rows(q16[[1, 2, 0]], k, lists)
    engine.dense_check()
    assert engine.dense_diag()["exhaustive"] >= 2
    ids, sc, ln = (a.cpu().numpy() for a in dev)
    for b in range(3):
        oid, osc = dense_exact_topk(x, q16[b], k)
        assert ln[b] == k and np.array_equal(ids[b], oid) and np.array_equal(_bits(sc[b]), _bits(osc)), b
    for got in (rows_host, tuple(a.cpu().numpy() for a in rows_dev)):
        for b, j in enumerate((1, 2, 0)):
            mask = np.zeros(n, bool)
            mask[lists[b]] = True
            oid, osc = dense_exact_topk(x, q16[j], k, mask)
            assert got[2][b] == k and np.array_equal(got[0][b], oid) and np.array_equal(_bits(got[1][b]), _bits(osc)), b
    assert engine.stat("dense_rows_calls") == 2
    # rows calls alone on a fresh handle: a check is a no-op that reports nothing exhaustive
    from easyrag_amd.engine import RetrievalEngine
    fresh = RetrievalEngine(0)
    try:
        fresh.set_dense(x[:5000])
        fresh.dense_topk_rows(q16, k, [np.arange(5000)], list_of=np.zeros(3, np.int32))
        fresh.dense_check()
        assert fresh.dense_diag()["exhaustive"] == 0 and fresh.stat("dense_exhaustive_queries") == 0
        assert fresh.stat("dense_rows_calls") == 1 and fresh.stat("dense_rows_long_launches") == 1
    finally:
        fresh.close()


def test_errors(engine):
    x = synth.dense_corpus(1000, 64, seed=1)
    engine.set_dense(x)
    q = x[:2]
    ok = [np.array([1, 5, 9]), np.array([2, 3])]
    st = _stats(engine)
    import ctypes as C

    def raw(rows, ptr, lo, k=3):
        """The C entry with arbitrary tables; outputs pre-filled so that 'untouched' can be seen."""
        rows, ptr, lo = np.asarray(rows, np.int32), np.asarray(ptr, np.int64), np.asarray(lo, np.int32)
        ids = np.full((2, max(k, 1)), 77, np.int32)
        sc = np.full((2, max(k, 1)), 7.5, np.float64)
        ln = np.full(2, 77, np.int32)
        rc = engine._lib.erh_dense_topk_rows(engine._h, q.ctypes.data, _lib.ERH_F16, 0, 0, 2, k, len(ptr) - 1, ptr.ctypes.data, rows.ctypes.data,
                                             lo.ctypes.data, ids.ctypes.data, sc.ctypes.data, ln.ctypes.data, 0, 0)
        return rc, bool(np.all(ids == 77) and np.all(sc == 7.5) and np.all(ln == 77))

    assert raw([1, 5, 9, 2, 3], [0, 3, 5], [0, 1])[0] == _lib.ERH_OK
    for rows, ptr, lo, who in (([5, 1, 9, 2, 3], [0, 3, 5], [0, 1], "unsorted"),
                               ([1, 5, 5, 2, 3], [0, 3, 5], [0, 1], "duplicate"),
                               ([1, 5, 1000, 2, 3], [0, 3, 5], [0, 1], "row == N"),
                               ([-1, 5, 9, 2, 3], [0, 3, 5], [0, 1], "negative row"),
                               ([1, 5, 9, 2, 3], [0, 4, 3], [0, 1], "list_ptr decreases"),
                               ([1, 5, 9, 2, 3], [0, 3, 5], [0, 2], "list_of == n_lists"),
                               ([1, 5, 9, 2, 3], [0, 3, 5], [-2, 1], "list_of < -1")):
        rc, untouched = raw(rows, ptr, lo)
        assert rc == _lib.ERH_ERR_INVALID and untouched, who
    for k in (0, 769):
        rc, untouched = raw([1, 5, 9, 2, 3], [0, 3, 5], [0, 1], k=k)
        assert rc == _lib.ERH_ERR_UNSUPPORTED and untouched, k
    assert _moved(engine, st)[0]["dense_rows_calls"] == 1                  # nothing of the refused calls was enqueued or counted
    with pytest.raises(_lib.ErhError, match="status -1"):
        engine.dense_topk_rows(q, 3, [np.array([4, 4])] * 2)
    with pytest.raises(_lib.ErhError, match="status -5"):
        engine.dense_topk_rows(q, 769, ok)
    from easyrag_amd.engine import RetrievalEngine
    fresh = RetrievalEngine(0)
    try:
        with pytest.raises(_lib.ErhError, match="status -4"):
            fresh.dense_topk_rows(q, 3, ok)                                  # no chunk matrix
    finally:
        fresh.close()
    assert C.sizeof(C.c_int64) == 8


# ---- retrievers and hybrid --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bm25_type", [0, 1])
def test_retrievers_with_rows(bm25_type):
    """QdrantRetriever.retrieve_batch(rows=) and score_nodes against the oracle's masked ranking; HybridRetriever(retrieval_type=3) with rows on
    the dense side against the oracle's RRF of the oracle's BM25 list and the masked dense list; rows_route_max > 0 == rows_route_max = 0 on
    the 103 questions of the fixture corpus, each filtered to its own dir."""
    import asyncio
    import zlib
    from conftest import WhitespaceTokenizer
    from test_reference_fixtures import DIRS, _fixture, synthetic_text_corpus
    from easyrag_amd.retrievers import BM25Retriever, HipVectorStore, HybridRetriever, QdrantRetriever
    from easyrag_amd.schema import TextNode
    from oracle import BM25Okapi, BM25SLucene, bm25_filter, reciprocal_rank_fusion
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
        hy = HybridRetriever(dense, sparse, retrieval_type=3, topk=10)
        queries = [" ".join(q["tokens"]) for q in fx["queries"]]
        docs = [tokenize_and_remove_stopwords(tok, t, stop) for t in texts]
        ora = BM25Okapi(docs, 1.5, 0.75, 0.25) if bm25_type == 0 else BM25SLucene(1.5, 0.75).index(docs)
        x16, dir_arr = to_f16_unit(vecs), np.array(dirs)
        n = len(nodes)
        cid = {}
        cid = [cid.setdefault(t, i) for i, t in enumerate(texts)]
        rng = np.random.default_rng(9)

        def pairs(lst):
            return [(g.node.node_id, g.score) for g in lst]

        def want_dense(query, rows, k=288):
            q16 = to_f16_unit(np.asarray(emb.get_query_embedding(query), np.float32))
            mask = None
            if rows is not None:
                mask = np.zeros(n, bool)
                mask[np.asarray(rows, np.int64)] = True
            return dense_exact_topk(x16, q16, k, mask)

        # QdrantRetriever: per-query rows, None entries, rows + filter, one array for all
        rows = [_pick(rng, n, 150), None, _pick(rng, n, 2500), _pick(rng, n, 40), None, _pick(rng, n, 700)]
        flts = [None, {"dir": "rcp"}, None, {"dir": "umac"}, None, {"dir": "rcp"}]
        eng.reset_stats()
        got = dense.retrieve_batch(queries[:6], filters=flts, rows=rows)
        assert eng.stat("dense_rows_calls") == 1 and eng.stat("dense_rows_short_launches") == 1 and eng.stat("dense_rows_long_launches") == 1
        assert eng.stat("dense_calls") == 1
        for b in range(6):
            allowed = np.arange(n) if rows[b] is None else rows[b]
            if flts[b]:
                allowed = allowed[dir_arr[allowed] == flts[b]["dir"]]
            did, dsc = want_dense(queries[b], None if (rows[b] is None and not flts[b]) else allowed)
            assert pairs(got[b]) == [(nodes[int(i)].node_id, float(s)) for i, s in zip(did, dsc)], b
        one = _pick(rng, n, 300)
        got = dense.retrieve_batch(queries[:3], rows=one)
        for b in range(3):
            did, dsc = want_dense(queries[b], one)
            assert pairs(got[b]) == [(nodes[int(i)].node_id, float(s)) for i, s in zip(did, dsc)], b
        # score_nodes: exactly the given nodes, all of them, ranked; more than one list's worth too
        for cnt in (192, 1000):
            given = _pick(rng, n, cnt)
            got = dense.score_nodes(queries[0], [nodes[int(i)] for i in given[:5]] + [int(i) for i in given[5:]])
            did, dsc = want_dense(queries[0], given, k=cnt)
            assert pairs(got) == [(nodes[int(i)].node_id, float(s)) for i, s in zip(did, dsc)], cnt
        assert pairs(dense.score_nodes(queries[0], given, top_k=7)) == pairs(got)[:7]

        # hybrid: rows on the dense side, filter_dict on the sparse side, one device pipeline
        own = [q["dir"] for q in fx["queries"]]
        B = len(queries)
        hrows = [_pick(rng, n, int(L)) for L in rng.integers(1, 900, B)]
        hrows[3] = hrows[2]                                                   # a shared list
        hrows[5] = _pick(rng, n, 2600)                                        # the long shape inside the fused call
        fds = [{"dir": d} if b % 2 == 0 else None for b, d in enumerate(own)]
        want_hy = []
        for b, (q, query) in enumerate(zip(fx["queries"], queries)):
            sp = bm25_filter(ora.get_scores(q["tokens"]), 192, None if fds[b] is None else dir_arr == own[b])
            did, dsc = want_dense(query, hrows[b])
            fused = reciprocal_rank_fusion([[Item(i, cid[i], s) for i, s in sp],
                                            [Item(int(i), cid[int(i)], float(s)) for i, s in zip(did, dsc)]], K=60, topk=10)
            want_hy.append([(nodes[w.idx].node_id, w.score) for w in fused])
        eng.reset_stats()
        batch = hy.retrieve_batch(queries, filter_dicts=fds, rows=hrows)
        assert eng.stat("hybrid_calls") == 0 and eng.stat("dense_calls") == 0 and eng.stat("bm25_calls") == 1 and eng.stat("dense_rows_calls") == 1
        for b in range(B):
            assert pairs(batch[b]) == want_hy[b], b
        mixed = list(hrows)
        mixed[1] = None                                                       # a batch that mixes rows and non-rows dense queries
        got = hy.retrieve_batch(queries[:4], filter_dicts=fds[:4], rows=mixed[:4])
        for b in (0, 2, 3):
            assert pairs(got[b]) == want_hy[b], b

        # rows_route_max: identical results on the 103 questions, each filtered to its own dir; the small dirs take the rows entry
        fown = [{"dir": d} for d in own]
        eng.reset_stats()
        base = dense.retrieve_batch(queries, filters=fown)
        assert eng.stat("dense_rows_calls") == 0
        store.rows_route_max = 1000
        routed = dense.retrieve_batch(queries, filters=fown)
        sizes = {d: int(np.sum(dir_arr == d)) for d in set(own)}
        assert eng.stat("dense_rows_calls") == (1 if any(v <= 1000 for v in sizes.values()) else 0), sizes
        store.rows_route_max = n
        routed_all = dense.retrieve_batch(queries, filters=fown)
        assert eng.stat("dense_rows_calls") >= 1
        store.rows_route_max = 0
        for b in range(B):
            assert pairs(base[b]) == pairs(routed[b]) == pairs(routed_all[b]), b
        hy.filter_dict = hy.filters = None
        assert asyncio.run(hy.aretrieve(queries[0])) is not None
    finally:
        sparse.close()
        eng.close()


# ---- full size: 1M x 1024, 5000 contiguous dirs of 200 rows, 1024 queries each on its own dir through rows -------------------------------
def test_full_size_1024_queries_each_on_its_own_200_row_dir(engine):
    import torch
    N, D, B, k = 1_000_000, 1024, 1024, 100
    dev = torch.device("cuda", 0)
    x = synth.dense_corpus_torch(N, D, seed=2, device=dev)
    q = synth.dense_queries_torch(x, B, seed=1000)
    engine.set_dense(x)
    engine.set_doc_meta(N, None, None)
    rng = np.random.default_rng(5)
    dirs = rng.choice(5000, size=B, replace=False)
    lists = [np.arange(200 * c, 200 * c + 200, dtype=np.int64) for c in dirs]
    q16 = q.cpu().numpy()
    engine.reset_stats()
    ids, sc, ln = engine.dense_topk_rows(q16, k, lists)
    assert engine.stat("dense_rows_calls") == 1 and engine.stat("dense_rows_short_launches") == 1 and engine.stat("dense_rows_long_launches") == 0
    assert np.all(ln == k)
    assert np.all((ids >= (200 * dirs)[:, None]) & (ids < (200 * dirs + 200)[:, None]))
    for b in range(0, B, B // 40)[:40]:
        xr = x[200 * dirs[b]: 200 * dirs[b] + 200].cpu().numpy()
        s = dense_exact_scores(xr, q16[b])
        oid, osc = _rank(np.concatenate([np.zeros(200 * dirs[b]), s]), lists[b], k)
        assert np.array_equal(ids[b], oid) and np.array_equal(_bits(sc[b]), _bits(osc)), b
