"""GPU parity, dense route with a SET of allowed classes per query (erh_dense_topk_sets): Qdrant filters with MatchAny / MatchExcept /
should / must_not, which the reference's QdrantRetriever hands to Qdrant unchanged (retrievers.py:44-47).  Every (query, class) pair
runs as a sub-query of one ordinary class-column batch and a merge kernel takes the top k of their union.  Results must equal the
oracle's masked ranking (ids, lengths, fp64 score bits) on every option arm, the canonical merge of the single-class answers in FAST
mode, and today's erh_dense_topk for the rows of a batch that carry no set."""
import numpy as np
import pytest

from easyrag_amd import _lib, synth
from oracle import dense_exact_topk, reciprocal_rank_fusion, to_f16_unit

pytestmark = pytest.mark.gpu

KS = (1, 7, 100, 288, 768)


def _bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


def _canon_merge(lists, k):
    """Canonical top k (score desc, index asc) of the union of (ids, scores) lists."""
    ids = np.concatenate([np.asarray(i, np.int64) for i, _ in lists]) if lists else np.zeros(0, np.int64)
    sc = np.concatenate([np.asarray(s, np.float64) for _, s in lists]) if lists else np.zeros(0)
    order = np.lexsort((ids, -sc))[:k]
    return ids[order], sc[order]


def _mask(dir_id, s):
    return None if s is None else np.isin(dir_id, np.asarray(s, np.int64))


def _check_oracle(x, q16, k, dir_id, sets, got, rows, cache=None):
    ids, sc, ln = got
    for i in rows:
        key = (i, None if sets[i] is None else tuple(sets[i]), k)
        if cache is not None and key in cache:
            oid, osc = cache[key]
        else:
            oid, osc = dense_exact_topk(x, q16[i], k, _mask(dir_id, sets[i]))
            if cache is not None:
                cache[key] = (oid, osc)
        assert ln[i] == len(oid), (i, sets[i])
        assert np.array_equal(ids[i, :ln[i]], oid), (i, sets[i])
        assert np.array_equal(_bits(sc[i, :ln[i]]), _bits(osc)), (i, sets[i])
        assert np.all(ids[i, ln[i]:] == -1) and np.all(sc[i, ln[i]:] == 0.0), i


def _random_sets(rng, B, n_classes):
    out = []
    for _ in range(B):
        m = int(rng.integers(2, n_classes))                       # 2 .. all - 1
        out.append([int(c) for c in rng.choice(n_classes, size=m, replace=False)])
    return out


@pytest.fixture(params=[(2, 1), (2, 0), (1, 1), (1, 0), (0, 1), (0, 0)],
                ids=["blocks2-grouped", "blocks2-per-group", "blocks1-grouped", "blocks1-per-group", "column-grouped", "column-per-group"])
def arm(engine, request):
    engine.set_option("dense_dir_blocks", request.param[0])
    engine.set_option("dense_group_launch", request.param[1])
    yield engine
    engine.set_option("dense_dir_blocks", 1)
    engine.set_option("dense_group_launch", 1)


_CORPORA = {}


def _corpus(kind):
    if kind not in _CORPORA:
        rng = np.random.default_rng(7 if kind == "contiguous" else 8)
        if kind == "contiguous":                                  # dirs as blocks of the caller's order, one below the block minimum
            sizes, d = [5000, 8000, 3000, 4500, 6000], 128
            dir_id = np.repeat(np.arange(len(sizes)), sizes).astype(np.int16)
        else:                                                     # dirs interleaved row by row
            n, d = 30000, 1024
            dir_id = rng.integers(0, 5, n).astype(np.int16)
        n = dir_id.shape[0]
        x = to_f16_unit(rng.standard_normal((n, d), dtype=np.float32))
        base = x[rng.integers(0, n, 12)].astype(np.float32)
        q16 = to_f16_unit(base + 0.6 * rng.standard_normal(base.shape).astype(np.float32) / np.sqrt(d))
        sets = _random_sets(rng, q16.shape[0], 5)
        _CORPORA[kind] = (x, q16, dir_id, sets, {})
    return _CORPORA[kind]


@pytest.mark.parametrize("kind", ["contiguous", "interleaved"])
def test_sets_match_oracle_on_every_arm(arm, kind):
    engine = arm
    x, q16, dir_id, sets, cache = _corpus(kind)
    engine.set_dense(x)
    engine.set_doc_meta(x.shape[0], None, dir_id)
    for k in KS:
        got = engine.dense_topk_sets(q16, k, sets)
        _check_oracle(x, q16, k, dir_id, sets, got, range(q16.shape[0]), cache)


def _expand(sets, n_classes_present):
    """The sub-query batch erh_dense_topk_sets builds: (row, class) per allowed class with documents, None -> (row, -1)."""
    rows, col, ptr = [], [], [0]
    for b, s in enumerate(sets):
        if s is None:
            rows.append(b); col.append(-1)
        else:
            for c in s:
                if 0 <= c < n_classes_present:
                    rows.append(b); col.append(c)
        ptr.append(len(rows))
    return np.asarray(rows, np.int64), np.asarray(col, np.int16), ptr


@pytest.mark.parametrize("kind", ["contiguous", "interleaved"])
def test_fast_mode_equals_merge_of_single_class_answers(engine, kind):
    x, q16, dir_id, sets, _ = _corpus(kind)
    engine.set_dense(x)
    engine.set_doc_meta(x.shape[0], None, dir_id)
    for k in (7, 288):
        ids, sc, ln = engine.dense_topk_sets(q16, k, sets, mode=_lib.ERH_DENSE_FAST)
        rows, col, ptr = _expand(sets, 5)
        sid, ssc, sln = engine.dense_topk(q16[rows], k, filter_dir=col, mode=_lib.ERH_DENSE_FAST)
        for b in range(q16.shape[0]):
            want = _canon_merge([(sid[j, :sln[j]], ssc[j, :sln[j]]) for j in range(ptr[b], ptr[b + 1])], k)
            assert ln[b] == len(want[0]) and np.array_equal(ids[b, :ln[b]], want[0]), b
            assert np.array_equal(_bits(sc[b, :ln[b]]), _bits(want[1])), b
            assert np.all(np.isin(dir_id[ids[b, :ln[b]]], sets[b]))


def test_degenerate_sets(engine):
    rng = np.random.default_rng(31)
    sizes, d, k = [9000, 7000, 5, 6000], 256, 100                # class 2 is smaller than k
    dir_id = np.repeat(np.arange(len(sizes)), sizes).astype(np.int16)
    n = dir_id.shape[0]
    x = to_f16_unit(rng.standard_normal((n, d), dtype=np.float32))
    q16 = to_f16_unit(rng.standard_normal((6, d), dtype=np.float32))
    engine.set_dense(x)
    engine.set_doc_meta(n, None, dir_id)
    col = np.asarray([1, 0, 3, 2, 1, 0], np.int16)
    want = engine.dense_topk(q16, k, filter_dir=col)
    got = engine.dense_topk_sets(q16, k, [[int(c)] for c in col])            # one class: erh_dense_topk with that column
    for a, b in zip(want, got):
        assert np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))
    plain = engine.dense_topk(q16, k)
    got = engine.dense_topk_sets(q16, k, [None] * 6)                         # {-1}: unfiltered
    for a, b in zip(plain, got):
        assert np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))
    ids, sc, ln = engine.dense_topk_sets(q16, k, [[], [0, 1], [], [2, 32767], [1, 32767], [2, 3]])
    assert ln[0] == 0 and ln[2] == 0 and np.all(ids[0] == -1) and np.all(sc[2] == 0.0)
    assert ln[3] == 5                                                        # a class smaller than k: a short sub-list
    one = engine.dense_topk(q16[4:5], k, filter_dir=np.asarray([1], np.int16))
    assert np.array_equal(ids[4], one[0][0]) and np.array_equal(_bits(sc[4]), _bits(one[1][0]))   # 32767 contributes nothing
    sets = [[], [0, 1], [], [2], [1], [2, 3]]
    _check_oracle(x, q16, k, dir_id, sets, (ids, sc, ln), range(6))
    with pytest.raises(_lib.ErhError, match="status -1"):
        engine.dense_topk_sets(q16[:1], k, [[1, 1]])                         # a class twice
    with pytest.raises(_lib.ErhError, match="status -1"):
        engine.dense_topk_sets(q16[:1], k, [[-1, 2]])
    with pytest.raises(_lib.ErhError, match="status -5"):
        engine.dense_topk_sets(q16[:1], 769, [[1, 2]])
    engine.set_doc_meta(n, None, None)
    with pytest.raises(_lib.ErhError, match="status -4"):
        engine.dense_topk_sets(q16[:1], k, [[1, 2]])
    assert engine.dense_topk_sets(q16[:1], k, [None])[2][0] == k             # {-1} needs no class column


def test_ties_across_classes_come_out_in_index_order(engine):
    rng = np.random.default_rng(41)
    n, d, k = 24000, 256, 50
    dir_id = (np.arange(n) % 3).astype(np.int16)                             # interleaved
    x = to_f16_unit(rng.standard_normal((n, d), dtype=np.float32))
    hot = x[5].copy()
    planted = np.sort(rng.choice(n, size=40, replace=False))
    x[planted] = hot                                                         # identical rows in all classes
    engine.set_dense(x)
    engine.set_doc_meta(n, None, dir_id)
    q16 = np.stack([hot, hot])
    sets = [[0, 2], [1, 2]]
    ids, sc, ln = engine.dense_topk_sets(q16, k, sets)
    _check_oracle(x, q16, k, dir_id, sets, (ids, sc, ln), range(2))
    for b in range(2):
        tied = ids[b, :ln[b]][sc[b, :ln[b]] == sc[b, 0]]
        assert len(tied) > 10 and np.all(np.diff(tied) > 0)


def test_device_outputs_and_the_exhaustive_path(engine):
    """device_out + erh_dense_check equals the host outputs; a set whose class holds 17000 exact copies of the query (more than the
    candidate budget: the sub-query is answered by the exhaustive path at the check) is still exact -- the merge runs again there."""
    import torch
    rng = np.random.default_rng(53)
    n, d, k = 40000, 256, 100
    dir_id = np.repeat(np.arange(3), [22000, 9000, 9000]).astype(np.int16)
    x = to_f16_unit(rng.standard_normal((n, d), dtype=np.float32))
    hot = to_f16_unit(rng.standard_normal((1, d), dtype=np.float32))[0]
    copies = np.sort(rng.choice(22000, size=17000, replace=False))
    x[copies] = hot
    engine.set_dense(x)
    engine.set_doc_meta(n, None, dir_id)
    q16 = np.stack([hot, to_f16_unit(rng.standard_normal((1, d), dtype=np.float32))[0], hot])
    sets = [[0, 1], [1, 2], [2, 0]]
    host = engine.dense_topk_sets(q16, k, sets)
    assert engine.dense_diag()["exhaustive"] >= 2
    _check_oracle(x, q16, k, dir_id, sets, host, range(3))
    assert np.array_equal(host[0][0], copies[:k])
    dev = engine.dense_topk_sets(torch.from_numpy(q16).cuda(), k, sets, device_out=True)
    engine.dense_check()
    assert engine.dense_diag()["exhaustive"] >= 2
    for a, b in zip(host, dev):
        assert np.array_equal(np.asarray(a).view(np.uint8), b.cpu().numpy().view(np.uint8))


def test_mixed_batch(engine):
    x, q16, dir_id, sets, cache = _corpus("interleaved")
    engine.set_dense(x)
    engine.set_doc_meta(x.shape[0], None, dir_id)
    B, k = q16.shape[0], 100
    mixed = [sets[b] if b % 3 == 0 else (None if b % 3 == 1 else [b % 5]) for b in range(B)]
    ids, sc, ln = engine.dense_topk_sets(q16, k, mixed)
    plain_rows = [b for b in range(B) if b % 3 != 0]
    col = np.asarray([-1 if mixed[b] is None else mixed[b][0] for b in plain_rows], np.int16)
    pid, psc, pln = engine.dense_topk(q16[plain_rows], k, filter_dir=col)
    assert np.array_equal(ids[plain_rows], pid) and np.array_equal(_bits(sc[plain_rows]), _bits(psc)) and np.array_equal(ln[plain_rows], pln)
    _check_oracle(x, q16, k, dir_id, mixed, (ids, sc, ln), range(B), cache)


# ---- full size: 1M x 1024, four dir blocks, 1024 queries --------------------------------------------------------------------------
def test_full_size_any_of_two_and_must_not_one(engine):
    import torch
    N, D, B, k = 1_000_000, 1024, 1024, 100
    dev = torch.device("cuda", 0)
    x = synth.dense_corpus_torch(N, D, seed=2, device=dev)
    q = synth.dense_queries_torch(x, B, seed=1000)
    dir_id = np.repeat(np.arange(4), N // 4).astype(np.int16)
    engine.set_dense(x)
    engine.set_doc_meta(N, None, dir_id)
    q16 = q.cpu().numpy()
    rng = np.random.default_rng(77)
    any2 = [sorted(int(c) for c in rng.choice(4, 2, replace=False)) for _ in range(B)]
    not1 = [[c for c in range(4) if c != b % 4] for b in range(B)]
    single = [engine.dense_topk(q16, k, filter_dir=np.full(B, c, np.int16)) for c in range(4)]
    from test_gpu_fullsize import dense_oracle_topk               # (pinned fp64 re-score of the fp32 candidates: the oracle at 1M rows)
    sample = list(range(0, B, B // 16))
    dir_dev = torch.from_numpy(dir_id).to(dev)
    for sets in (any2, not1):
        ids, sc, ln = engine.dense_topk_sets(q16, k, sets)
        for b in range(B):
            want = _canon_merge([(single[c][0][b, :single[c][2][b]], single[c][1][b, :single[c][2][b]]) for c in sets[b]], k)
            assert ln[b] == k and np.array_equal(ids[b], want[0]) and np.array_equal(_bits(sc[b]), _bits(want[1])), b
        allowed = [torch.isin(dir_dev, torch.tensor(sets[b], device=dev, dtype=dir_dev.dtype)) for b in sample]
        for b, (oid, osc) in zip(sample, dense_oracle_topk(x, q[sample], k, allowed)):
            assert np.array_equal(ids[b], oid) and np.array_equal(_bits(sc[b]), _bits(osc)), b


# ---- retrievers and hybrid --------------------------------------------------------------------------------------------------------
class _MatchValue:
    def __init__(self, value):
        self.value = value


class _MatchAny:
    def __init__(self, any):
        self.any = any


class _FieldCondition:
    def __init__(self, key, match=None, range=None):
        self.key, self.match, self.range = key, match, range


class _Filter:
    def __init__(self, must=None, should=None, must_not=None):
        self.must, self.should, self.must_not, self.min_should = must, should, must_not, None


def _any(key, vals):
    return _Filter(must=[_FieldCondition(key, match=_MatchAny(list(vals)))])


def test_retrievers_and_hybrid_with_set_filters():
    """QdrantRetriever with a MatchAny `filters`, per-query lists of mixed filter objects through HipVectorStore.query_batch, and
    HybridRetriever(retrieval_type=3) with a set `filters` and a dict `filter_dict` against the oracle composition; then the reference's
    103 questions, each allowed its own document plus one other, as one batch = the 103 single aretrieve calls = the oracle."""
    import asyncio
    import zlib
    from conftest import WhitespaceTokenizer
    from test_reference_fixtures import DIRS, _fixture
    from easyrag_amd.retrievers import BM25Retriever, HipVectorStore, HybridRetriever, QdrantRetriever
    from easyrag_amd.schema import TextNode
    from oracle import BM25Okapi, bm25_filter
    from oracle.retrievers import Item, tokenize_and_remove_stopwords

    class Embedder:
        def get_query_embedding(self, text, d=256):
            v = np.random.default_rng(zlib.crc32(text.encode())).standard_normal(d).astype(np.float32)
            return (v / np.linalg.norm(v)).tolist()

    from test_reference_fixtures import synthetic_text_corpus
    fx = _fixture()
    texts, dirs = synthetic_text_corpus(fx, n_docs=5000)
    order = np.argsort(np.array([DIRS.index(d) for d in dirs]), kind="stable")
    texts, dirs = [texts[i] for i in order], [dirs[i] for i in order]
    texts[40] = texts[11]
    nodes = [TextNode(text=t, metadata={"dir": d}, id_=f"n{i}") for i, (t, d) in enumerate(zip(texts, dirs))]
    emb, tok, stop = Embedder(), WhitespaceTokenizer(), {""}
    vecs = np.asarray([emb.get_query_embedding(f"doc{i}:" + t) for i, t in enumerate(texts)], np.float32)
    sparse = BM25Retriever.from_defaults(nodes=nodes, tokenizer=tok, similarity_top_k=192, stopwords=stop, bm25_type=0)
    eng = sparse.engine
    try:
        store = HipVectorStore(nodes, vecs, engine=eng)
        dense = QdrantRetriever(store, emb, similarity_top_k=288)
        hy = HybridRetriever(dense, sparse, retrieval_type=3, topk=10)
        eng.set_option("dense_dir_block_min_rows", 1)
        queries = [" ".join(q["tokens"]) for q in fx["queries"]]
        docs = [tokenize_and_remove_stopwords(tok, t, stop) for t in texts]
        ora = BM25Okapi(docs, 1.5, 0.75, 0.25)
        x16, dir_arr = to_f16_unit(vecs), np.array(dirs)
        cid = {}
        cid = [cid.setdefault(t, i) for i, t in enumerate(texts)]

        def pairs(lst):
            return [(g.node.node_id, g.score) for g in lst]

        def want_dense(query, allowed):
            q16 = to_f16_unit(np.asarray(emb.get_query_embedding(query), np.float32))
            did, dsc = dense_exact_topk(x16, q16, 288, None if allowed is None else np.isin(dir_arr, allowed))
            return did, dsc

        # QdrantRetriever with a MatchAny filters attribute
        dense.filters = _any("dir", ["rcp", "umac"])
        got = dense.retrieve_batch(queries[:6])
        for b in range(6):
            did, dsc = want_dense(queries[b], ["rcp", "umac"])
            assert pairs(got[b]) == [(nodes[int(i)].node_id, float(s)) for i, s in zip(did, dsc)], b
        assert pairs(asyncio.run(dense.aretrieve(queries[0]))) == pairs(got[0])
        dense.filters = None
        # per-query mixed filter objects through the store
        flts = [None, {"dir": "rcp"}, _any("dir", ["director", "emsplus"]), _Filter(must_not=[_FieldCondition("dir", _MatchValue("umac"))]),
                _Filter(should=[_FieldCondition("dir", _MatchValue("rcp")), _FieldCondition("dir", _MatchValue("umac"))])]
        allowed = [None, ["rcp"], ["director", "emsplus"], ["rcp", "director", "emsplus"], ["rcp", "umac"]]
        embs = np.asarray([emb.get_query_embedding(q) for q in queries[:5]], np.float32)
        ids, sc, ln = store.query_batch(embs, 288, filters=flts)
        for b in range(5):
            did, dsc = want_dense(queries[b], allowed[b])
            assert np.array_equal(ids[b, :ln[b]], did) and np.array_equal(_bits(sc[b, :ln[b]]), _bits(dsc)), b

        # the 103 questions: own document + one other each, dense set filter + sparse dict filter, one batch
        own = [q["dir"] for q in fx["queries"]]
        other = [DIRS[(DIRS.index(d) + 1 + i % 3) % len(DIRS)] for i, d in enumerate(own)]
        fsets = [_any("dir", [a, b]) for a, b in zip(own, other)]
        fds = [{"dir": d} for d in own]
        want_hy = []
        for q, query, a, b2 in zip(fx["queries"], queries, own, other):
            sp = bm25_filter(ora.get_scores(q["tokens"]), 192, dir_arr == a)
            did, dsc = want_dense(query, [a, b2])
            fused = reciprocal_rank_fusion([[Item(i, cid[i], s) for i, s in sp],
                                            [Item(int(i), cid[int(i)], float(s)) for i, s in zip(did, dsc)]], K=60, topk=10)
            want_hy.append([(nodes[w.idx].node_id, w.score) for w in fused])
        for blocks in (2, 0):
            eng.set_option("dense_dir_blocks", blocks)
            eng.reset_stats()
            batch = hy.retrieve_batch(queries, filter_dicts=fds, filters=fsets)
            assert eng.stat("hybrid_calls") == 0 and eng.stat("dense_calls") == 1 and eng.stat("bm25_calls") == 1   # the device path
            for b in range(len(queries)):
                assert pairs(batch[b]) == want_hy[b], (blocks, b)
        eng.set_option("dense_dir_blocks", 1)
        for b, query in enumerate(queries):
            hy.filter_dict, hy.filters = fds[b], fsets[b]
            assert pairs(asyncio.run(hy.aretrieve(query))) == want_hy[b], b
        hy.filter_dict = hy.filters = None
    finally:
        sparse.close()
        eng.close()
