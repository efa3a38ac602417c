"""Fused route with hybrid_lazy: the dense route's final kernel re-scores only the rows the fused top-k can see (DESIGN K1).
Every case compares ids, fp64 scores and lengths EXACTLY between hybrid_lazy = 1, hybrid_lazy = 0 (the full re-score) and the oracle
composition bm25_filter + dense_exact_topk + reciprocal_rank_fusion.  Shapes are small on purpose: 6 000 - 10 000 chunks, d = 128 / 256,
B = 37 queries (no tile multiple), k_dense 288, k_sparse 192."""
import numpy as np
import pytest

from easyrag_amd.engine import queries_to_csr
from easyrag_amd.index import BM25S, build_bm25_index
from oracle import BM25SLucene, bm25_filter, dense_exact_topk, reciprocal_rank_fusion, to_f16_unit
from oracle.dense import dense_exact_scores
from oracle.retrievers import Item

pytestmark = pytest.mark.gpu

KD, KS, B = 288, 192, 37
VOCAB = 600                       # ordinary tokens; token VOCAB + b is query b's own (it occurs only where a test plants it)


class Scene:
    """A corpus on both routes + the oracle's route lists, computed once and shared by the tests that use the scene."""

    def __init__(self, x, docs, queries, q16, cid=None, dir_id=None, filt=None):
        self.x, self.docs, self.queries, self.q16, self.cid, self.dir_id, self.filt = x, docs, queries, q16, cid, dir_id, filt
        self.n = x.shape[0]
        self.idx = build_bm25_index(docs, BM25S)
        ora = BM25SLucene(k1=1.5, b=0.75).index(docs)
        self.o_sparse, self.o_dense = [], []
        for b, q in enumerate(queries):
            mask = None if filt is None or filt[b] < 0 else dir_id == filt[b]
            sc = ora.get_scores(q) if len(q) else np.zeros(self.n, np.float32)
            self.o_sparse.append(bm25_filter(sc, KS, mask))
            self.o_dense.append(dense_exact_topk(x, q16[b], KD, mask))
        self.csr = queries_to_csr([self.idx.tokens_to_ids(q) for q in queries])

    def key(self, i):
        return int(i) if self.cid is None else int(self.cid[i])

    def want(self, b, topk, K):
        A = [Item(i, self.key(i), s) for i, s in self.o_sparse[b]]
        D = [Item(int(i), self.key(i), float(s)) for i, s in zip(*self.o_dense[b])]
        return reciprocal_rank_fusion([A, D], K=K, topk=topk)

    def load(self, engine):
        engine.set_dense(self.x)
        engine.set_bm25(self.idx)
        engine.set_doc_meta(self.n, self.cid, self.dir_id)

    def run(self, engine, lazy, topk=10, K=60, rows=None):
        engine.set_option("hybrid_lazy", 2 if lazy else 0)  # (2: also where the default keeps the full path -- batches beside a side stream)
        try:
            sel = slice(None) if rows is None else rows
            csr = self.csr if rows is None else queries_to_csr([self.idx.tokens_to_ids(self.queries[b]) for b in rows])
            f = None if self.filt is None else self.filt[sel]
            return engine.hybrid_topk(self.q16[sel], *csr, k_dense=KD, k_sparse=KS, K=K, topk=topk, filter_dir=f)
        finally:
            engine.set_option("hybrid_lazy", 1)

    def three_way(self, engine, topk=10, K=60):
        """lazy on == lazy off == oracle, exactly; returns the two calls' counters."""
        out, st = {}, {}
        for lazy in (1, 0):
            engine.reset_stats()
            out[lazy] = self.run(engine, lazy, topk, K)
            st[lazy] = {"rows": engine.stat("dense_rescored_rows_last_call"), "lazy_queries": engine.stat("hybrid_lazy_queries"),
                        "exhaustive": engine.stat("dense_exhaustive_queries"), "grouped": engine.stat("dense_grouped_launches")}
        for lazy in (1, 0):
            ids, sc, ln = out[lazy]
            for b in range(len(self.queries)):
                want = self.want(b, topk, K)
                assert ln[b] == len(want), (lazy, b)
                assert list(ids[b, :ln[b]]) == [w.idx for w in want], f"hybrid_lazy={lazy} query {b}: fused ids differ"
                assert list(sc[b, :ln[b]]) == [w.score for w in want], f"hybrid_lazy={lazy} query {b}: fused scores differ"
        for a, c in zip(out[1], out[0]):
            a, c = np.asarray(a), np.asarray(c)
            assert np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a, c.view(np.uint64) if c.dtype == np.float64 else c)
        assert st[0]["lazy_queries"] == 0
        return st


def _tokens(rng, n, lo=8, hi=30):
    p = 1.0 / np.arange(1, VOCAB + 1) ** 1.07
    p /= p.sum()
    return [list(map(int, rng.choice(VOCAB, size=int(rng.integers(lo, hi)), p=p))) for _ in range(n)]


def _base(seed, n=6000, d=128):
    rng = np.random.default_rng(seed)
    x32 = rng.standard_normal((n, d)).astype(np.float32)
    docs = _tokens(rng, n)
    src = rng.integers(0, n, B)
    q32 = x32[src] + 0.5 * rng.standard_normal((B, d)).astype(np.float32)
    queries = [[int(t) for t in rng.choice(docs[int(rng.integers(0, n))], size=5)] + [VOCAB + b] for b in range(B)]
    return rng, x32, docs, q32, queries


_SCENES = {}


def _scene(name):
    if name not in _SCENES:
        _SCENES[name] = globals()["_make_" + name]()
    return _SCENES[name]


def _make_independent():
    """Case 1: the routes draw their targets independently (query b's own token occurs nowhere), no content ids."""
    rng, x32, docs, q32, queries = _base(11)
    return Scene(to_f16_unit(x32), docs, queries, to_f16_unit(q32))


def _make_correlated():
    """Case 2: each query's token targets and dense near-copies are the SAME 60 documents, spread over the dense ranks."""
    rng, x32, docs, q32, queries = _base(12)
    n, d = x32.shape
    for b in range(B):
        tgt = rng.choice(n, size=60, replace=False)
        noise = np.linspace(0.3, 1.6, 60)[:, None] * rng.standard_normal((60, d))
        x32[tgt] = (q32[b] + noise * np.linalg.norm(q32[b]) / np.sqrt(d) * 3.0).astype(np.float32)
        for t in tgt:
            docs[t] = docs[t] + [VOCAB + b] * int(rng.integers(1, 4))
    return Scene(to_f16_unit(x32), docs, queries, to_f16_unit(q32))


def _delta(s, b):
    """The kernel's delta = d * 2^-23 * |q| * max|x| for query b; the factor covers the fp32 rounding of its two norms (<= 1e-6 relative)."""
    x64, q64 = s.x.astype(np.float64), s.q16[b].astype(np.float64)
    return s.x.shape[1] * 2.0 ** -23 * np.linalg.norm(q64) * np.sqrt((x64 * x64).sum(1).max()) * (1.0 + 1e-5)


def _rows_bound(s, b, topk=10, K=60):
    """Issue bound from the oracle's fp64 scores with 4 delta margins: |{e >= e_(R_q) - 4 delta}| + sum over the joined documents (sparse
    list documents inside the margin set, e >= e_(kk) - 4 delta) of |{|e - e_j| <= 4 delta}|.  No content ids: M = 1, r* = topk."""
    e = dense_exact_scores(s.x, s.q16[b])
    dl = _delta(s, b)
    srt = np.sort(e)[::-1]
    assert len(s.o_sparse[b]) >= topk
    rq = 1 * (topk + K) - K
    bound = int((e >= srt[rq - 1] - 4 * dl).sum())
    for i, _ in s.o_sparse[b]:
        if e[i] >= srt[KD - 1] - 4 * dl:
            bound += int((np.abs(e - e[i]) <= 4 * dl).sum())
    return bound


def _per_query_bound(engine, s):
    """Case 9, per query: the counter is a sum over the call's queries, so every query is asked again on its own (same lists, same answer)
    and its re-scored rows are held against ITS bound."""
    for b in range(B):
        ids, sc, ln = s.run(engine, 1, rows=[b])
        rows, bound = engine.stat("dense_rescored_rows_last_call"), _rows_bound(s, b)
        assert 0 < rows <= bound, (b, rows, bound)
        want = s.want(b, 10, 60)
        assert list(ids[0, :ln[0]]) == [w.idx for w in want] and list(sc[0, :ln[0]]) == [w.score for w in want], b


def test_independent_routes(engine):
    s = _scene("independent")
    s.load(engine)
    st = s.three_way(engine)
    assert st[1]["lazy_queries"] == B                      # case 9: every query's need set is smaller than its margin set
    assert st[1]["rows"] < st[0]["rows"]
    assert st[0]["rows"] >= B * KD                         # (the full path re-scores the margin set: at least k_dense rows per query)
    _per_query_bound(engine, s)
    engine.reset_stats()                                   # the default (option 1) takes the lazy path at this batch size, not at one query per call
    engine.hybrid_topk(s.q16, *s.csr, k_dense=KD, k_sparse=KS, K=60, topk=10)
    assert engine.stat("hybrid_lazy_queries") == B
    engine.hybrid_topk(s.q16[:1], *queries_to_csr([s.idx.tokens_to_ids(s.queries[0])]), k_dense=KD, k_sparse=KS, K=60, topk=10)
    assert engine.stat("hybrid_lazy_queries") == B


def test_correlated_routes(engine):
    s = _scene("correlated")
    for b in range(B):                                     # on the oracle lists: the join is not empty
        joined = set(i for i, _ in s.o_sparse[b]) & set(int(i) for i in s.o_dense[b][0])
        assert len(joined) >= 20, (b, len(joined))
    s.load(engine)
    st = s.three_way(engine)
    assert st[1]["rows"] < st[0]["rows"]
    _per_query_bound(engine, s)


def _make_ties():
    """Case 3: exact duplicates (equal scores: the index decides) and rows that differ in one small element, around rank t = 10, around joined
    documents deep in the list, and across the k_dense-th position; part of them carry the query's own token (they are in the sparse list)."""
    rng, x32, docs, q32, queries = _base(13)
    x, q16 = to_f16_unit(x32), to_f16_unit(q32)
    used = set()
    for b in range(0, B, 3):
        order, _ = dense_exact_topk(x, q16[b], KD + 12)
        for r in (8, 57, 140, 251, 283, 287):              # 0-based: r = 8 straddles rank t = 10, r = 287 the k_dense-th position
            a, dup, near = (int(order[r]), int(order[r + 1]), int(order[r + 2]))
            if {a, dup, near} & used:
                continue
            used |= {a, dup, near}
            x[dup] = x[a]                                  # ties with a; the lower index ranks first
            x[near] = x[a]
            j = int(np.argmin(np.abs(x[a].astype(np.float32))))
            x[near, j] = np.nextafter(x[near, j], np.float16(1.0))      # one ulp of the row's smallest element
            for t in ((a, near) if r % 2 else (dup,)):
                docs[t] = docs[t] + [VOCAB + b]
    return Scene(x, docs, queries, q16)


def test_ties_and_near_ties(engine):
    s = _scene("ties")
    ties_at_k = 0
    for b in range(0, B, 3):
        _, sc = dense_exact_topk(s.x, s.q16[b], KD + 12)
        ties_at_k += int(sc[KD - 1] == sc[KD])             # a tie across the k_dense-th position: the index decides who is listed
        assert (np.diff(sc[:KD + 4]) == 0).sum() >= 3, b
        assert len(set(i for i, _ in s.o_sparse[b]) & set(int(i) for i in s.o_dense[b][0])) >= 3, b
    assert ties_at_k >= 3
    s.load(engine)
    st = s.three_way(engine)
    assert st[1]["lazy_queries"] == B


def _make_contents(mult):
    """Case 4: contents shared by `mult` documents.  For every third query the key of one of its best dense documents has its other occurrences
    deep in the dense list only (ranks 150 ... 280), half of them also in the sparse list; mult = 50: one content of 50 documents besides."""
    rng, x32, docs, q32, queries = _base(14 + mult)
    x, q16 = to_f16_unit(x32), to_f16_unit(q32)
    n = x.shape[0]
    cid = np.arange(n, dtype=np.int32)
    taken = set()
    per = min(mult, 3)
    if mult == 50:
        grp = rng.choice(n, size=50, replace=False)
        cid[grp] = cid[grp].min()
        taken |= set(int(i) for i in grp)
    for b in range(0, B, 3):
        order, _ = dense_exact_topk(x, q16[b], KD)
        members = [int(order[r]) for r in ((b // 3) % 3, 150 + b, 240 + b)[:per]]
        if set(members) & taken:
            continue
        taken |= set(members)
        cid[members] = min(members)
        if b % 2:
            docs[members[-1]] = docs[members[-1]] + [VOCAB + b]
    assert np.bincount(cid).max() == mult
    return Scene(x, docs, queries, q16, cid=cid)


@pytest.mark.parametrize("mult", [2, 3, 50])
def test_content_ids(engine, mult):
    if ("contents", mult) not in _SCENES:
        _SCENES[("contents", mult)] = _make_contents(mult)
    s = _SCENES[("contents", mult)]
    seen = 0
    for b in range(0, B, 3):                               # the shared key is in the fused top-10 with its deep occurrence counted
        deep = [int(i) for i in s.o_dense[b][0][100:] if (s.cid == s.cid[i]).sum() >= 2 and s.cid[i] in [w.content for w in s.want(b, 10, 60)]]
        seen += bool(deep)
    assert seen >= 5
    s.load(engine)
    st = s.three_way(engine)
    if mult == 50:
        assert st[1]["lazy_queries"] == 0 and st[1]["rows"] == st[0]["rows"]      # R_q >= k_dense: the full path
    else:
        assert st[1]["lazy_queries"] == B and st[1]["rows"] < st[0]["rows"]


def _make_short():
    """Case 5: (a) a query of unknown tokens, (b) sparse lists of fewer than t keys, (c) a dir that leaves fewer than k_dense candidates."""
    rng, x32, docs, q32, queries = _base(15)
    n = x32.shape[0]
    queries[3] = [VOCAB + 500, VOCAB + 501]                # (a) nothing matches: an empty sparse list
    for b in (4, 5):                                       # (b) the query's own token only, in 4 documents
        queries[b] = [VOCAB + b]
        for t in rng.choice(n, size=4, replace=False):
            docs[t] = docs[t] + [VOCAB + b]
    dir_id = np.zeros(n, np.int16)
    dir_id[rng.choice(n, size=150, replace=False)] = 1     # (c) 150 < k_dense documents
    filt = np.full(B, -1, np.int16)
    filt[[6, 7, 20]] = 1
    filt[8] = 0
    return Scene(to_f16_unit(x32), docs, queries, to_f16_unit(q32), dir_id=dir_id, filt=filt)


def test_short_lists(engine):
    s = _scene("short")
    assert len(s.o_sparse[3]) == 0 and 0 < len(s.o_sparse[4]) < 10 and len(s.o_dense[6][0]) == 150
    s.load(engine)
    st = s.three_way(engine)
    assert 0 < st[1]["lazy_queries"] <= B - 3              # (a), (b): the whole margin set


@pytest.mark.parametrize("topk,K,overlap", [(256, 60, -1), (10, 0, -1), (10, 7, -1), (10, 60, 0), (10, 60, 1), (10, 60, 2)])
def test_parameters(engine, topk, K, overlap):
    s = _scene("correlated")
    s.load(engine)
    engine.set_option("hybrid_overlap", overlap)
    try:
        st = s.three_way(engine, topk, K)
    finally:
        engine.set_option("hybrid_overlap", -1)
    if overlap == 2:
        assert st[1]["lazy_queries"] == 0                  # overlap 2 keeps the full path (the sparse route starts behind the scan)
    elif topk == 10:
        assert st[1]["lazy_queries"] == B                  # R_q = 10 whatever K is (no content ids)


def _make_blocks():
    """Case 7: two dirs of 4500 and 5500 rows, every query filtered on one of them: two block groups in ONE grouped launch."""
    rng, x32, docs, q32, queries = _base(17, n=10000, d=256)
    n = x32.shape[0]
    for b in range(B):
        for t in rng.choice(n, size=40, replace=False):
            docs[t] = docs[t] + [VOCAB + b]
    x, q16 = to_f16_unit(x32), to_f16_unit(q32)
    dir_id = np.repeat(np.arange(2), [4500, 5500]).astype(np.int16)
    filt = (np.arange(B) % 2).astype(np.int16)
    for b in range(B):                                     # joined documents inside the query's dir
        order, _ = dense_exact_topk(x, q16[b], KD, dir_id == filt[b])
        for r in (5, 30, 100, 200, 270):
            docs[int(order[r])] = docs[int(order[r])] + [VOCAB + b] * 3
    return Scene(x, docs, queries, q16, dir_id=dir_id, filt=filt)


def test_dir_filter_grouped_launch(engine):
    s = _scene("blocks")
    s.load(engine)
    engine.set_option("dense_dir_blocks", 2)
    try:
        st = s.three_way(engine)
        assert st[1]["grouped"] > 0 and st[0]["grouped"] > 0
        assert st[1]["lazy_queries"] == B and st[1]["rows"] < st[0]["rows"]
        # one query = one routed group run as a pipeline of its own
        ids, sc, ln = s.run(engine, 1, rows=[3])
        want = s.want(3, 10, 60)
        assert list(ids[0, :ln[0]]) == [w.idx for w in want] and list(sc[0, :ln[0]]) == [w.score for w in want]
    finally:
        engine.set_option("dense_dir_blocks", 1)


def test_queries_that_leave_the_pruned_pipeline(engine):
    """Case 8: the construction of test_gpu_dense.py::test_dense_speculation_failure_is_caught, fused -- the stored prefix holds exactly what
    some queries ask for (no row placement), their speculative threshold fails, the exhaustive path answers them with plain lists that
    the redone fusion reads beside the other queries' (id, rank) rows."""
    rng = np.random.default_rng(77)
    n, d = 10000, 256
    topic = rng.standard_normal(d)
    x32 = rng.standard_normal((n, d))
    x32[:200] = topic + 0.2 * rng.standard_normal((200, d))          # 200 < k_dense rows on topic, all inside the first n0 rows
    q32 = x32[rng.integers(200, n, B)] + 0.5 * rng.standard_normal((B, d))
    q32[:6] = topic + 0.2 * rng.standard_normal((6, d))
    docs = _tokens(rng, n)
    queries = [[int(t) for t in rng.choice(docs[int(rng.integers(0, n))], size=5)] for b in range(B)]
    s = Scene(to_f16_unit(x32), docs, queries, to_f16_unit(q32))
    engine.set_option("dense_n0", 512)
    engine.set_option("dense_shuffle", 0)
    try:
        s.load(engine)
        st = s.three_way(engine)
        assert st[1]["exhaustive"] > 0 and st[0]["exhaustive"] > 0
        assert st[1]["lazy_queries"] > 0
    finally:
        engine.set_option("dense_shuffle", 1)
        engine.set_option("dense_n0", 32768)
