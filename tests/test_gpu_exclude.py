"""GPU parity, exclude lists on every route (erh_dense_topk_excl / erh_bm25_topk_excl, csrc/exclude.hip, DESIGN K12): query b ranks what it may
see EXCEPT its exclusion list.  Ids AND fp64 score bits must equal the oracle's masked ranking with the mask
`allowed & ~np.isin(arange(N), excl)` -- dense: dense_exact_topk(x, q16, k, mask); sparse: bm25_filter(get_scores(q), k, keep_mask=mask).

The oracle's rankings are drawn from ONE score vector per query (dense_exact_scores / get_scores), computed once per module and left
unchanged; `_rank_dense` / test_gpu_bm25_sets._rank order the masked rows of that vector as the oracle functions do, and are held against
dense_exact_topk / bm25_filter literally inside the sweeps.

ERH_DENSE_FAST ranks by the scan's fp32 score, which no fp64 oracle reproduces bit for bit (the existing FAST tests compare it with the
library's own single-class answers for the same reason): there the reference is the mode's own ranking -- erh_dense_topk_sets in FAST
mode at depth k + e_max with the excluded ids removed on the host, in order, first k -- ids and score bits.

Exclusion pattern "every other id of its top 2k": 2k is capped so that k + (ids excluded) stays within the entry's depth (768 / 1024)."""
from dataclasses import dataclass, field
from typing import Any, List

import numpy as np
import pytest

import test_gpu_bm25_sets as sets_mod
from conftest import make_text_corpus
from easyrag_amd import _lib
from easyrag_amd.engine import RetrievalEngine, live_device_bytes
from easyrag_amd.index import BM25S, OKAPI
from easyrag_amd.retrievers import (BM25Retriever, HipVectorStore, HybridRetriever, QdrantRetriever,
                                    tokenize_and_remove_stopwords)
from easyrag_amd.schema import TextNode
from oracle import BM25Okapi, bm25_filter, dense_exact_topk, reciprocal_rank_fusion, to_f16_unit
from oracle.dense import dense_exact_scores
from oracle.retrievers import Item

pytestmark = pytest.mark.gpu

STATS = ("dense_excl_calls", "bm25_excl_calls", "excl_drop_launches", "dense_rows_calls", "bm25_rows_calls", "dense_calls", "bm25_calls")


def _bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


def _host(got):
    return tuple(a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a) for a in got)


def _stats(engine):
    return {n: engine.stat(n) for n in STATS}


def _moved(engine, before):
    after = _stats(engine)
    return {n: after[n] - before[n] for n in after if after[n] != before[n]}


def _check_lists(got, want, k, who=""):
    """got: (ids, sc, len) of a call; want[b] = (ids, scores) of the oracle: lengths, ids, score bits, padding."""
    ids, sc, ln = _host(got)
    B = len(want)
    assert ids.shape == (B, k) and sc.shape == (B, k) and ln.shape == (B,)
    for b, (oid, osc) in enumerate(want):
        assert ln[b] == len(oid), (who, b, int(ln[b]), len(oid))
        assert np.array_equal(ids[b, :ln[b]], oid), (who, b)
        assert np.array_equal(_bits(sc[b, :ln[b]]), _bits(osc)), (who, b)
        assert np.all(ids[b, ln[b]:] == -1) and np.all(_bits(sc[b, ln[b]:]) == 0), (who, b)


# ---- dense --------------------------------------------------------------------------------------------------------------------------------
DN, DD, DB = 3000, 64, 9
D_SIZES = (1000, 800, 600, 400, 150, 45, 5)        # seven classes of unequal size, class 6 has 5 rows
D_KS = (1, 10, 63, 64, 65, 100)
# query b's class set: None = the set {-1}
D_SETS = [None, None, [0, 1], [2, 3, 6], [0, 6], [1, 2, 3, 4, 5], None, [4, 5, 6], [5, 6]]
# query b's exclusion pattern
D_PATTERNS = ["nothing", "rank1", "top5", "top64", "every-other", "outside", "top64", "every-other", "class6"]

_DENSE = {}


def _dense_corpus():
    """Matrix, class column, nine queries and their exact score vectors [9 x N], computed once and left unchanged."""
    if not _DENSE:
        rng = np.random.default_rng(41)
        dir_id = rng.permutation(np.repeat(np.arange(7), D_SIZES)).astype(np.int16)
        x = to_f16_unit(rng.standard_normal((DN, DD), dtype=np.float32))
        base = x[rng.integers(0, DN, DB)].astype(np.float32)
        q16 = to_f16_unit(base + 0.6 * rng.standard_normal(base.shape).astype(np.float32) / np.sqrt(DD))
        S = np.stack([dense_exact_scores(x, q16[b]) for b in range(DB)])
        _DENSE.update(x=x, q16=q16, dir_id=dir_id, S=S)
    return _DENSE


def _rank_dense(s, mask, k):
    """dense_exact_topk's ranking of one score vector: (score desc, index asc) over the masked rows, first k."""
    idx = np.flatnonzero(mask)
    order = np.lexsort((idx, -s[idx]))[:k]
    return idx[order].astype(np.int64), s[idx][order]


def _allowed_mask(dir_id, st):
    return np.ones(dir_id.shape[0], bool) if st is None else np.isin(dir_id, np.asarray(st, np.int64))


def _pattern(name, ranked_ids, k, limit, dir_id, st):
    """One exclusion list.  ranked_ids: the query's oracle ranking of its allowed rows (all of them)."""
    if name == "nothing":
        return np.zeros(0, np.int64)
    if name == "rank1":
        return ranked_ids[:1]
    if name in ("top5", "top64"):
        return ranked_ids[:int(name[3:])]
    if name == "every-other":
        return ranked_ids[:2 * min(k, limit - k):2]
    if name == "outside":                              # ids the query cannot see anyway
        return np.flatnonzero(~_allowed_mask(dir_id, st))[:40]
    if name == "class6":
        return np.flatnonzero(dir_id == 6)
    raise AssertionError(name)


def _dense_case(c, k, sets):
    """Exclusion lists and the oracle's masked rankings of the nine queries at this k."""
    excl, want = [], []
    for b in range(DB):
        allowed = _allowed_mask(c["dir_id"], sets[b])
        ranked, _ = _rank_dense(c["S"][b], allowed, DN)
        e = np.sort(_pattern(D_PATTERNS[b], ranked, k, 768, c["dir_id"], sets[b]))
        excl.append(e)
        want.append(_rank_dense(c["S"][b], allowed & ~np.isin(np.arange(DN), e), k))
    return excl, want


@pytest.fixture
def dense_engine(engine):
    c = _dense_corpus()
    engine.set_dense(c["x"])
    engine.set_doc_meta(DN, None, c["dir_id"])
    yield engine
    engine.set_doc_meta(DN, None, None)


def test_dense_oracle_sweep(dense_engine):
    import torch
    engine, c = dense_engine, _dense_corpus()
    q_dev = torch.from_numpy(c["q16"]).cuda()
    for k in D_KS:
        for sets in (D_SETS, None):                    # class sets with {-1} among them / set_ptr NULL
            per_query = D_SETS if sets is not None else [None] * DB
            excl, want = _dense_case(c, k, per_query)
            st = _stats(engine)
            host = engine.dense_topk_excl(c["q16"], k, excl, sets=sets)
            assert _moved(engine, st) == {"dense_excl_calls": 1, "excl_drop_launches": 1}
            _check_lists(host, want, k, ("dense", k, sets is None))
            dev = engine.dense_topk_excl(q_dev, k, excl, sets=sets, device_out=True)
            engine.sync()                              # no dense_check: the entry checked its inner call itself
            for a, b in zip(_host(dev), host):
                assert np.array_equal(a.view(np.uint8), np.asarray(b).view(np.uint8)), ("device outputs", k)
        if k == 100:
            ln = np.asarray(host[2])
            assert ln[8] == 100 and ln[0] == 100       # (unfiltered call: class 6 gone, everything else left)
    # filtered: the query on classes {5, 6} without class 6 has 45 rows left
    excl, want = _dense_case(c, 100, D_SETS)
    got = engine.dense_topk_excl(c["q16"], 100, excl, sets=D_SETS)
    assert np.asarray(got[2])[8] == 45 and len(want[8][0]) == 45
    # the helper against the literal oracle call
    for b in (1, 3, 8):
        mask = _allowed_mask(c["dir_id"], D_SETS[b]) & ~np.isin(np.arange(DN), excl[b])
        oid, osc = dense_exact_topk(c["x"], c["q16"][b], 100, mask)
        assert np.array_equal(oid, want[b][0]) and np.array_equal(_bits(osc), _bits(want[b][1])), b


def test_dense_fast_mode_is_the_modes_own_ranking(dense_engine):
    engine, c = dense_engine, _dense_corpus()
    for k in D_KS:
        excl, _ = _dense_case(c, k, D_SETS)
        kk = k + max(e.size for e in excl)
        ids, sc, ln = engine.dense_topk_sets(c["q16"], kk, D_SETS, mode=_lib.ERH_DENSE_FAST)
        want = []
        for b in range(DB):
            keep = ~np.isin(ids[b, :ln[b]], excl[b])
            want.append((ids[b, :ln[b]][keep][:k], sc[b, :ln[b]][keep][:k]))
        got = engine.dense_topk_excl(c["q16"], k, excl, sets=D_SETS, mode=_lib.ERH_DENSE_FAST)
        _check_lists(got, want, k, ("fast", k))


def _raw_dense(engine, q16, k, eptr, eids, fill=-7):
    """erh_dense_topk_excl on caller-filled host outputs: (status, outputs untouched)."""
    B = q16.shape[0]
    ids, sc, ln = np.full((B, k), fill, np.int32), np.full((B, k), float(fill)), np.full(B, fill, np.int32)
    eptr, eids = np.ascontiguousarray(eptr, np.int32), np.ascontiguousarray(eids, np.int32)
    rc = engine._lib.erh_dense_topk_excl(engine._h, q16.ctypes.data, _lib.ERH_F16, 0, 0, B, k, None, None, eptr.ctypes.data,
                                         eids.ctypes.data if eids.size else None, _lib.ERH_DENSE_EXACT, ids.ctypes.data, sc.ctypes.data,
                                         ln.ctypes.data, 0, None)
    return rc, bool(np.all(ids == fill) and np.all(sc == float(fill)) and np.all(ln == fill)), (ids, sc, ln)


def _raw_bm25(engine, qi, qt, k, eptr, eids, fill=-7):
    B = qi.shape[0] - 1
    ids, sc, ln = np.full((B, k), fill, np.int32), np.full((B, k), float(fill)), np.full(B, fill, np.int32)
    eptr, eids = np.ascontiguousarray(eptr, np.int32), np.ascontiguousarray(eids, np.int32)
    rc = engine._lib.erh_bm25_topk_excl(engine._h, qi.ctypes.data, qt.ctypes.data, B, k, None, None, eptr.ctypes.data,
                                        eids.ctypes.data if eids.size else None, ids.ctypes.data, sc.ctypes.data, ln.ctypes.data, 0, None)
    return rc, bool(np.all(ids == fill) and np.all(sc == float(fill)) and np.all(ln == fill)), (ids, sc, ln)


def test_dense_depth_limit(dense_engine):
    engine, c = dense_engine, _dense_corpus()
    q16 = np.ascontiguousarray(c["q16"][:2])
    everything = np.ones(DN, bool)
    ranked = _rank_dense(c["S"][1], everything, DN)[0]
    e = np.sort(ranked[:68])                           # kk = 700 + 68 = 768 exactly
    got = engine.dense_topk_excl(q16, 700, [None, e])
    want = [_rank_dense(c["S"][0], everything, 700), _rank_dense(c["S"][1], ~np.isin(np.arange(DN), e), 700)]
    _check_lists(got, want, 700, "kk = 768")
    e = np.sort(ranked[:69])                           # kk = 769
    rc, untouched, _ = _raw_dense(engine, q16, 700, [0, 0, 69], e)
    assert rc == _lib.ERH_ERR_UNSUPPORTED and untouched
    assert "769" in engine._lib.erh_last_error(engine._h).decode()
    with pytest.raises(_lib.ErhError) as err:
        engine.dense_topk_excl(q16, 769, None)
    assert err.value.status == _lib.ERH_ERR_UNSUPPORTED


def test_dense_refuses_while_a_check_is_pending(dense_engine):
    import torch
    engine, c = dense_engine, _dense_corpus()
    k = 10
    excl, want = _dense_case(c, k, [None] * DB)
    q_dev = torch.from_numpy(c["q16"]).cuda()
    first = engine.dense_topk(q_dev, k, device_out=True)            # waits for its dense_check
    with pytest.raises(_lib.ErhError) as err:
        engine.dense_topk_excl(c["q16"], k, excl)
    assert err.value.status == _lib.ERH_ERR_STATE
    engine.dense_check()
    _check_lists(engine.dense_topk_excl(c["q16"], k, excl), want, k, "after the check")
    engine.sync()
    everything = np.ones(DN, bool)
    _check_lists(first, [_rank_dense(c["S"][b], everything, k) for b in range(DB)], k, "the earlier call")


def test_dense_empty_exclusions_equal_the_sets_entry(dense_engine):
    engine, c = dense_engine, _dense_corpus()
    for k in (1, 65, 100):
        a = engine.dense_topk_sets(c["q16"], k, D_SETS)
        b = engine.dense_topk_excl(c["q16"], k, None, sets=D_SETS)
        for x, y in zip(a, b):
            assert np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8)), k


# ---- sparse -------------------------------------------------------------------------------------------------------------------------------
S_KS = (1, 10, 192, 960)
SN, SQ = sets_mod.N, sets_mod.NQ
S_SETS = [None, None, [0, 1], [2, 3, 7], [0, 7], [1, 2, 3, 4, 5], None, [4, 5, 7], [5, 7], None, [0, 1, 2], None, None, None]
S_PATTERNS = ["nothing", "rank1", "top5", "top64", "every-other", "outside", "top64", "every-other", "class7", "top5", "rank1", "top64",
              "all-positive", "nothing"]            # query 12: the rare-term query, query 13: the empty query

_SPARSE = {}


def _sparse_corpus(variant):
    """test_gpu_bm25_sets' corpus (N = 6000, vocabulary 2000) and its twelve queries, plus a query of one rare term and an empty one;
    score vectors [14 x N], computed once per variant and left unchanged."""
    if variant not in _SPARSE:
        c = sets_mod._corpus(variant)
        df = {}
        for d in c["docs"]:
            for t in set(d):
                df[t] = df.get(t, 0) + 1
        rare = min(t for t, n in df.items() if 5 <= n <= 40)
        queries = list(c["queries"]) + [[rare], []]
        S = np.concatenate([c["S"], sets_mod._scores(c["ora"], [rare], SN)[None], np.zeros((1, SN))])
        assert 5 <= int((S[12] > 0).sum()) <= 40
        _SPARSE[variant] = dict(idx=c["idx"], ora=c["ora"], queries=queries, S=S)
    return _SPARSE[variant]


def _sparse_case(c, k, sets, dir_id):
    excl, want = [], []
    for b in range(len(sets)):
        allowed = _allowed_mask(dir_id, sets[b])
        ranked, _ = sets_mod._rank(c["S"][b], np.flatnonzero(allowed), SN)
        name = S_PATTERNS[b]
        if name == "all-positive":
            e = np.flatnonzero(c["S"][b] > 0)
        elif name == "class7":
            e = np.flatnonzero(dir_id == 7)
        else:
            e = _pattern(name, ranked, k, 1024, dir_id, sets[b])
        e = np.sort(e)
        excl.append(e)
        want.append(sets_mod._rank(c["S"][b], np.flatnonzero(allowed & ~np.isin(np.arange(SN), e)), k))
    return excl, want


@pytest.fixture
def sparse_meta(engine):
    dir_id = sets_mod._layout("blocks")                 # class 7: five documents
    engine.set_doc_meta(SN, None, dir_id)
    yield dir_id
    engine.set_doc_meta(SN, None, None)


@pytest.mark.parametrize("variant", [OKAPI, BM25S])
def test_sparse_oracle_sweep(engine, sparse_meta, variant):
    c, dir_id = _sparse_corpus(variant), sparse_meta
    engine.set_bm25(c["idx"])
    csr = sets_mod._csr(c["idx"], c["queries"])
    B = len(c["queries"])
    for k in S_KS:
        for sets in (S_SETS, None):
            per_query = S_SETS if sets is not None else [None] * B
            excl, want = _sparse_case(c, k, per_query, dir_id)
            if k == 960:
                assert k + max(e.size for e in excl) == 1024        # the depth limit exactly
            st = _stats(engine)
            host = engine.bm25_topk_excl(*csr, k, excl, sets=sets)
            assert _moved(engine, st) == {"bm25_excl_calls": 1, "excl_drop_launches": 1}
            _check_lists(host, want, k, ("sparse", variant, k, sets is None))
            assert np.asarray(host[2])[12] == 0 and np.asarray(host[2])[13] == 0
            dev = engine.bm25_topk_excl(*csr, k, excl, sets=sets, device_out=True)
            engine.sync()
            for a, b in zip(_host(dev), host):
                assert np.array_equal(a.view(np.uint8), np.asarray(b).view(np.uint8)), ("device outputs", k)
    # the helper against the literal oracle walk
    excl, want = _sparse_case(c, 192, S_SETS, dir_id)
    for b in (1, 3, 7, 8):
        mask = _allowed_mask(dir_id, S_SETS[b]) & ~np.isin(np.arange(SN), excl[b])
        lit = bm25_filter(c["ora"].get_scores(c["queries"][b]), 192, mask)
        assert [w[0] for w in lit] == list(want[b][0]) and np.array_equal(_bits([w[1] for w in lit]), _bits(want[b][1])), b
    # kk = 1025 is refused
    qi, qt = csr
    e = np.arange(65, dtype=np.int32)
    eptr = np.zeros(B + 1, np.int32)
    eptr[1:] = 65
    rc, untouched, _ = _raw_bm25(engine, qi, qt, 960, eptr, e)
    assert rc == _lib.ERH_ERR_UNSUPPORTED and untouched and "1025" in engine._lib.erh_last_error(engine._h).decode()
    with pytest.raises(_lib.ErhError) as err:
        engine.bm25_topk_excl(qi, qt, 0, None)
    assert err.value.status == _lib.ERH_ERR_UNSUPPORTED


# ---- malformed lists ----------------------------------------------------------------------------------------------------------------------
MALFORMED = [("unsorted", [0, 2, 2], [5, 3]), ("duplicated", [0, 2, 2], [3, 3]), ("too large", [0, 1, 1], [None]), ("negative", [0, 1, 1], [-1]),
             ("decreasing pointer", [0, 2, 1], [1, 2]), ("pointer not from 0", [1, 2, 2], [1, 2])]


def test_malformed_lists_are_refused_on_both_entries(dense_engine):
    engine, c = dense_engine, _dense_corpus()
    sc = _sparse_corpus(OKAPI)
    engine.set_bm25(sc["idx"])
    q16 = np.ascontiguousarray(c["q16"][:2])
    qi, qt = sets_mod._csr(sc["idx"], sc["queries"][:2])
    k = 10
    for what, eptr, eids in MALFORMED:
        for n, raw, args in ((DN, _raw_dense, (q16,)), (SN, _raw_bm25, (qi, qt))):
            ids = [n if x is None else x for x in eids]
            rc, untouched, _ = raw(engine, *args, k, eptr, ids)
            assert rc == _lib.ERH_ERR_INVALID and untouched, (what, raw.__name__)
    rc, untouched, _ = _raw_dense(engine, q16, k, [0, 0, 0], [])     # a null excl_ids with nothing excluded is fine
    assert rc == _lib.ERH_OK and not untouched
    # a following valid call is correct
    everything = np.ones(DN, bool)
    e = [np.sort(_rank_dense(c["S"][b], everything, 3)[0]) for b in range(2)]
    _check_lists(engine.dense_topk_excl(q16, k, e), [_rank_dense(c["S"][b], ~np.isin(np.arange(DN), e[b]), k) for b in range(2)], k, "dense")
    e = [np.sort(sets_mod._rank(sc["S"][b], np.arange(SN), 3)[0]) for b in range(2)]
    _check_lists(engine.bm25_topk_excl(qi, qt, k, e),
                 [sets_mod._rank(sc["S"][b], np.flatnonzero(~np.isin(np.arange(SN), e[b])), k) for b in range(2)], k, "sparse")


def test_live_bytes_return():
    import gc
    c, sc = _dense_corpus(), _sparse_corpus(BM25S)
    gc.collect()
    base = live_device_bytes()
    eng = RetrievalEngine(0)
    try:
        eng.set_dense(c["x"])
        eng.set_bm25(sc["idx"])
        excl, want = _dense_case(c, 10, [None] * DB)
        _check_lists(eng.dense_topk_excl(c["q16"], 10, excl), want, 10, "fresh handle")
        qi, qt = sets_mod._csr(sc["idx"], sc["queries"][:2])
        got = eng.bm25_topk_excl(qi, qt, 10, [[1, 2], None])
        assert got[0].shape == (2, 10)
        assert eng.stat("excl_drop_launches") == 2 and live_device_bytes() - base > 0
    finally:
        eng.close()
    assert live_device_bytes() - base == 0


# ---- retrievers and the hybrid ------------------------------------------------------------------------------------------------------------
@dataclass
class HasIdCondition:
    has_id: List[Any] = field(default_factory=list)


@dataclass
class Filter:
    should: Any = None
    min_should: Any = None
    must: Any = None
    must_not: Any = None


@pytest.fixture(scope="module")
def node_corpus(tokenizer):
    """The small node corpus of test_gpu_retrievers.py, its retrievers on one engine, and the oracle's score vectors of three queries."""
    from test_gpu_retrievers import STOP, FakeEmbedder
    texts = make_text_corpus(1200, 150, seed=7)
    texts[100] = texts[7]
    texts[900] = texts[7]
    dirs = ["umac", "rcp", "director", "emsplus"]
    nodes = [TextNode(text=t, metadata={"dir": dirs[i % 4], "know_path": f"kp {i % 9}"}, id_=f"n{i}") for i, t in enumerate(texts)]
    emb = FakeEmbedder()
    vecs = np.asarray([emb.get_query_embedding("doc:" + t + str(i)) for i, t in enumerate(texts)], np.float32)
    sparse = BM25Retriever.from_defaults(nodes=nodes, tokenizer=tokenizer, similarity_top_k=192, stopwords=STOP, bm25_type=0)
    store = HipVectorStore(nodes, vecs, engine=sparse.engine)
    dense = QdrantRetriever(store, emb, similarity_top_k=288)
    x16 = to_f16_unit(vecs)
    ora = BM25Okapi([tokenize_and_remove_stopwords(tokenizer, n.get_content(), STOP) for n in nodes], 1.5, 0.75, 0.25)
    queries = ["w5 w9 w3", "w14 w2 w2 w60 w8", "w7 w21"]
    SS = [np.asarray(ora.get_scores(tokenize_and_remove_stopwords(tokenizer, q, STOP)), np.float64) for q in queries]
    DS = [dense_exact_scores(x16, to_f16_unit(np.asarray(emb.get_query_embedding(q), np.float32))) for q in queries]
    key = {}
    cid = [key.setdefault(n.get_content(), i) for i, n in enumerate(nodes)]
    is_rcp = np.array([n.metadata["dir"] == "rcp" for n in nodes])
    yield dict(nodes=nodes, sparse=sparse, dense=dense, queries=queries, SS=SS, DS=DS, cid=cid, is_rcp=is_rcp, n=len(nodes))
    sparse.close()


def _node_ids(lst):
    return [g.node.node_id for g in lst]


@pytest.mark.parametrize("filtered", [False, True])
def test_hybrid_equals_the_fusion_of_the_masked_lists(node_corpus, filtered):
    c = node_corpus
    n, nodes, B = c["n"], c["nodes"], len(c["queries"])
    hy = HybridRetriever(c["dense"], c["sparse"], retrieval_type=3, topk=256)
    allowed = c["is_rcp"] if filtered else np.ones(n, bool)
    # per query: its best sparse and dense rows, as positions, node ids, nodes -- one form each
    tops = [np.concatenate([sets_mod._rank(c["SS"][b], np.flatnonzero(allowed), 7)[0], _rank_dense(c["DS"][b], allowed, 9)[0]]) for b in range(B)]
    exclude = [tops[0], [nodes[i].node_id for i in tops[1]], [nodes[i] for i in tops[2]]]
    kw = dict(filter_dicts=[{"dir": "rcp"}] * B, filters=[{"dir": "rcp"}] * B) if filtered else {}
    eng = c["sparse"].engine
    st = _stats(eng)
    got = hy.retrieve_batch(c["queries"], exclude=exclude, **kw)
    assert _moved(eng, st) == {"dense_excl_calls": 1, "bm25_excl_calls": 1, "excl_drop_launches": 2}
    for b in range(B):
        mask = allowed & ~np.isin(np.arange(n), tops[b])
        A = [Item(i, c["cid"][i], s) for i, s in bm25_filter(c["SS"][b], 192, mask)]
        did, dsc = _rank_dense(c["DS"][b], mask, 288)
        want = reciprocal_rank_fusion([A, [Item(int(i), c["cid"][int(i)], float(s)) for i, s in zip(did, dsc)]], topk=256)
        assert _node_ids(got[b]) == [nodes[w.idx].node_id for w in want], b
        assert [g.score for g in got[b]] == [w.score for w in want], b
    # must_not: [HasIdCondition] on both routes is the same question
    f = [Filter(must_not=[HasIdCondition(has_id=[int(i) for i in tops[b]])]) for b in range(B)]
    if not filtered:
        via = hy.retrieve_batch(c["queries"], filters=f, sparse_filters=f)
        assert [_node_ids(x) for x in via] == [_node_ids(x) for x in got]


@pytest.mark.parametrize("route", ["dense", "sparse"])
def test_paging_reproduces_one_deep_call(node_corpus, route):
    c = node_corpus
    r = c[route]
    keep, eng = r._similarity_top_k, c["sparse"].engine
    try:
        r._similarity_top_k = 200
        deep = r.retrieve_batch(c["queries"])
        r._similarity_top_k = 50
        shown = [[] for _ in c["queries"]]
        for p in range(4):                                 # page p excludes the pages in front of it
            st = _stats(eng)
            page = r.retrieve_batch(c["queries"], exclude=shown)
            assert _moved(eng, st).get("dense_excl_calls" if route == "dense" else "bm25_excl_calls", 0) == (1 if p else 0)
            shown = [s + p for s, p in zip(shown, page)]
    finally:
        r._similarity_top_k = keep
    for b in range(len(c["queries"])):
        assert _node_ids(shown[b]) == _node_ids(deep[b][:200]) and len(shown[b]) == min(200, len(deep[b])), (route, b)
        assert np.array_equal(_bits([g.score for g in shown[b]]), _bits([g.score for g in deep[b][:200]])), (route, b)


def test_long_exclusions_take_the_complement_route(node_corpus):
    c = node_corpus
    n, nodes, eng = c["n"], c["nodes"], c["sparse"].engine
    everything = np.ones(n, bool)
    q = c["queries"][:2]
    # dense: 288 + 500 > 768
    excl = [_rank_dense(c["DS"][b], everything, 500)[0] for b in range(2)]
    st = _stats(eng)
    got = c["dense"].retrieve_batch(q, exclude=excl)
    assert _moved(eng, st) == {"dense_rows_calls": 1}
    for b in range(2):
        oid, osc = _rank_dense(c["DS"][b], ~np.isin(np.arange(n), excl[b]), 288)
        assert _node_ids(got[b]) == [nodes[i].node_id for i in oid] and np.array_equal(_bits([g.score for g in got[b]]), _bits(osc)), b
    # sparse: 192 + 900 > 1024 (the best 900 positive documents, filled up with others where a query has fewer)
    excl = [np.concatenate([sets_mod._rank(c["SS"][b], np.arange(n), 900)[0], np.flatnonzero(c["SS"][b] <= 0)])[:900] for b in range(2)]
    assert all(np.unique(e).size == 900 for e in excl)
    st = _stats(eng)
    got = c["sparse"].retrieve_batch(q, exclude=excl)
    assert _moved(eng, st) == {"bm25_rows_calls": 1}
    for b in range(2):
        oid, osc = sets_mod._rank(c["SS"][b], np.flatnonzero(~np.isin(np.arange(n), excl[b])), 192)
        assert _node_ids(got[b]) == [nodes[i].node_id for i in oid] and np.array_equal(_bits([g.score for g in got[b]]), _bits(osc)), b
