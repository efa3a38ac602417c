"""GPU: the fusion kernels, the classmethods' device branch and the retrievers on the composition corpus against answers
produced by the REFERENCE's own glue (tests/golden/ref_glue*.{json,npz}; see tests/golden/make_ref_glue_fixture.py).
Reads nothing but tests/golden/.  Nodes are compared by identity / index, scores by their float64 bits."""
import numpy as np
import pytest

import oracle
from _ref_glue import bits, composition_texts, fuse_cases, load, rrf_K
from easyrag_amd.engine import RetrievalEngine
from easyrag_amd.retrievers import BM25Retriever, HipVectorStore, HybridRetriever, QdrantRetriever
from easyrag_amd.schema import TextNode
from oracle.retrievers import Item
from test_ref_glue_fixture import _shim_fuse, check_fused

pytestmark = pytest.mark.gpu

KERNEL_MAX_ITEMS = 2048


def test_fusion_kernels_match_reference_in_one_launch():
    """erh_rrf / erh_fusion: every two-list case the kernel takes, rows of different lengths (0 included) packed into one
    launch; ids, lengths and fp64 score bits, at the full length and cut."""
    cases = [c for c in fuse_cases() if len(c[3]) in (1, 2) and sum(c[3]) <= KERNEL_MAX_ITEMS]
    rows = []
    off = 0
    for name, cid, sc, lens, modes in cases:
        la, lb = lens[0], (lens[1] if len(lens) > 1 else 0)
        rows.append((name, off, la, lb, cid, sc, modes))
        off += la + lb
    assert any(r[2] == 0 for r in rows) and any(r[3] == 0 for r in rows)
    B, da, db = len(rows), max(r[2] for r in rows), max(r[3] for r in rows)
    content = np.empty(off, np.int32)
    coff = 0
    ia, ib = np.full((B, max(da, 1)), -1, np.int32), np.full((B, max(db, 1)), -1, np.int32)
    sa, sb = np.zeros(ia.shape), np.zeros(ib.shape)
    la, lb = np.zeros(B, np.int32), np.zeros(B, np.int32)
    for b, (name, o, na, nb, cid, sc, _) in enumerate(rows):
        content[o:o + na + nb] = coff + cid                       # content ids of different rows never meet
        coff += int(cid.max()) + 1 if len(cid) else 0
        ia[b, :na], ib[b, :nb] = np.arange(o, o + na), np.arange(o + na, o + na + nb)
        sa[b, :na], sb[b, :nb] = sc[:na], sc[na:]
        la[b], lb[b] = na, nb
    n_distinct = max(len(set(r[4].tolist())) for r in rows)
    eng = RetrievalEngine(0)
    try:
        eng.set_doc_meta(off, content, None)
        for m in ("fusion", "rrf_K0", "rrf_K1", "rrf_K60", "rrf_K1000003"):
            for topk in (n_distinct, 1, 7, 256):
                if rrf_K(m) is None:
                    ids, osc, ln = eng.fusion(ia, sa, la, ib, sb, lb, topk=topk)
                else:
                    ids, osc, ln = eng.rrf(ia, la, ib, lb, K=rrf_K(m), topk=topk)
                for b, (name, o, na, nb, cid, sc, modes) in enumerate(rows):
                    pos, want_sc, _ = modes[m]
                    n = min(topk, len(pos))
                    assert int(ln[b]) == n, (name, m, topk)
                    assert (ids[b, :n] - o).tolist() == pos[:n].tolist(), (name, m, topk)
                    assert bits(osc[b, :n]).tolist() == bits(want_sc[:n]).tolist(), (name, m, topk)
    finally:
        eng.close()


def test_classmethod_device_branch_matches_reference():
    """HybridRetriever.fusion / .reciprocal_rank_fusion above fusion_device_min items (the kernels' branch, up to 2048) and
    beyond: returned nodes, score bits, topk <= 0 slicing, and the RRF score written into EVERY fused input node."""
    n = 0
    for name, cid, sc, lens, modes in fuse_cases():
        if sum(lens) <= HybridRetriever.fusion_device_min:
            continue
        n += 1
        for m, (pos, osc, topk_len) in modes.items():
            for topk, ln in topk_len.items():
                got = _shim_fuse(cid, sc, lens, rrf_K(m), topk)
                check_fused(*got, sc, pos, osc, ln, rrf_K(m) is not None, (name, m, topk))
    assert n == 4                                  # 513, 2047, 2048 (device) and 2049 (host) items


# ---------------------------------------------------------------------------------------------------------------------
# the composition corpus
class _Embedder:
    def __init__(self, queries, emb):
        assert len(set(queries)) == len(queries)
        self.by_text = {q: e for q, e in zip(queries, emb)}

    def get_query_embedding(self, text):
        return self.by_text[text].tolist()


@pytest.fixture(scope="module")
def comp(tokenizer):
    data, _, z = load()
    texts, meta, queries, qfilt = composition_texts()
    nodes = [TextNode(text=t, metadata=m, id_=f"n{i}") for i, (t, m) in enumerate(zip(texts, meta))]
    toks_c = [t.split(" ") for t in texts]
    toks_p = [m["know_path"].split(" ") for m in meta]
    ora = {0: (oracle.BM25Okapi(toks_c, 1.5, 0.75, 0.25), oracle.BM25Okapi(toks_p, 1.5, 0.75, 0.25)),
           1: (oracle.BM25SLucene(1.5, 0.75).index(toks_c), oracle.BM25SLucene(1.5, 0.75).index(toks_p))}
    return dict(data=data["composition"], z=z, nodes=nodes, queries=queries, qfilt=qfilt, ora=ora,
                emb=_Embedder(queries, z["query_emb_f32"]))


def _ids(out, nodes):
    index = {id(n): i for i, n in enumerate(nodes)}
    return [[index[id(g.node)] for g in row] for row in out]


def _want_filter(c, bt, qn, k):
    full = c["z"][f"filter_t{bt}_ids"][qn]
    n = int(c["z"][f"filter_t{bt}_lens"][qn][c["data"]["filter_ks"].index(k)])
    return full[full >= 0][:n].tolist()


@pytest.mark.parametrize("bm25_type", [0, 1])
def test_bm25_retriever_composition(comp, tokenizer, bm25_type):
    nodes, queries, qfilt = comp["nodes"], comp["queries"], comp["qfilt"]
    r = BM25Retriever.from_defaults(nodes=nodes, tokenizer=tokenizer, similarity_top_k=6, bm25_type=bm25_type)
    try:
        scores = [comp["ora"][bm25_type][0].get_scores(q.split(" ")) for q in queries]
        for k in comp["data"]["filter_ks"]:          # 0 and 1100 lie outside erh_bm25_topk: the host filter answers
            r._similarity_top_k = k
            got = r.retrieve_batch(queries, filter_dicts=qfilt)
            for qn, row in enumerate(got):
                assert _ids([row], nodes)[0] == _want_filter(comp, bm25_type, qn, k), (k, qn)
                assert bits([g.score for g in row]).tolist() == bits([float(scores[qn][i]) for i in _ids([row], nodes)[0]]).tolist()
            # the scalar knob: one filter_dict for a batch of the queries that carry it
            fd = next(f for f in qfilt if f)
            sub = [qn for qn, f in enumerate(qfilt) if f == fd]
            r.filter_dict = fd
            got = r.retrieve_batch([queries[qn] for qn in sub])
            r.filter_dict = None
            assert _ids(got, nodes) == [_want_filter(comp, bm25_type, qn, k) for qn in sub], k
    finally:
        r.close()


def _hybrid(comp, tokenizer, shared: bool, k_sparse=192):
    sparse = BM25Retriever.from_defaults(nodes=comp["nodes"], tokenizer=tokenizer, similarity_top_k=k_sparse, bm25_type=0)
    eng = sparse.engine if shared else RetrievalEngine(0)
    store = HipVectorStore(comp["nodes"], comp["z"]["doc_emb_f16"], engine=eng)
    dense = QdrantRetriever(store, comp["emb"], similarity_top_k=comp["data"]["k_dense"])
    return sparse, dense, (None if shared else eng)


@pytest.mark.parametrize("shared", [True, False], ids=["fused", "unfused"])
def test_hybrid_retriever_composition(comp, tokenizer, shared):
    z, nodes, queries, qfilt = comp["z"], comp["nodes"], comp["queries"], comp["qfilt"]
    sparse, dense, extra = _hybrid(comp, tokenizer, shared)
    try:
        topk = comp["data"]["topk_rrf"]
        for rt in (1, 2, 3):
            h = HybridRetriever(dense, sparse, retrieval_type=rt, topk=topk)
            assert h._fused_possible() == shared
            got = _ids(h.retrieve_batch(queries, filter_dicts=qfilt, filters=qfilt), nodes)
            for qn in range(len(queries)):
                if rt == 1:
                    assert got[qn] == z["dense_ids"][qn].tolist(), qn
                elif rt == 2:
                    assert got[qn] == _want_filter(comp, 0, qn, 192), qn
                else:
                    n = int(z["rrf_len"][qn])
                    assert got[qn] == z["rrf_ids"][qn, :n].tolist(), qn
        out = h.retrieve_batch(queries, filter_dicts=qfilt, filters=qfilt)
        for qn, row in enumerate(out):
            n = int(z["rrf_len"][qn])
            assert bits([g.score for g in row]).tolist() == bits(z["rrf_scores"][qn, :n]).tolist(), qn
        # topk <= 0: the reference slices [:topk] after fusing; the fused kernel takes topk >= 1 only, the routes answer
        h = HybridRetriever(dense, sparse, retrieval_type=3, topk=0)
        assert h.retrieve_batch(queries[:4], filter_dicts=qfilt[:4], filters=qfilt[:4]) == [[], [], [], []]
        h.topk = -1
        for qn, row in enumerate(h.retrieve_batch(queries[:4], filter_dicts=qfilt[:4], filters=qfilt[:4])):
            n = int(z["rrf_len"][qn])
            assert _ids([row], nodes)[0][:n] == z["rrf_ids"][qn, :n].tolist()
        # dense k above 768 has no exact fall-back: an error that names the limit
        dense._similarity_top_k = 769
        with pytest.raises(ValueError, match="768"):
            h.retrieve_batch(queries[:1])
        dense._similarity_top_k = comp["data"]["k_dense"]
    finally:
        sparse.close()
        if extra is not None:
            extra.close()


def test_hybrid_sparse_k_above_kernel_limit(comp, tokenizer):
    """k_sparse 1100 > erh_hybrid_topk's 1024: the shared-engine retriever takes the separate routes (BM25 through the host
    filter) and still answers what the reference answers with the whole filtered sparse list."""
    z, nodes, queries, qfilt = comp["z"], comp["nodes"], comp["queries"], comp["qfilt"]
    sparse, dense, _ = _hybrid(comp, tokenizer, True, k_sparse=1100)
    try:
        h = HybridRetriever(dense, sparse, retrieval_type=3, topk=256)
        got = _ids(h.retrieve_batch(queries, filter_dicts=qfilt, filters=qfilt), nodes)
        key = {}
        cid = [key.setdefault(n.get_content(), i) for i, n in enumerate(nodes)]
        for qn in range(len(queries)):
            sp = _want_filter(comp, 0, qn, 1100)
            want = oracle.reciprocal_rank_fusion([[Item(i, cid[i], 0.0) for i in sp],
                                                  [Item(int(i), cid[int(i)], 0.0) for i in z["dense_ids"][qn]]], topk=256)
            assert got[qn] == [w.idx for w in want], qn
    finally:
        sparse.close()


@pytest.mark.parametrize("bm25_type", [0, 1])
def test_shipped_yaml_fusion_composition(comp, tokenizer, bm25_type):
    """pipeline.py:201-208, 357-365: fusion([content route top 192, know_path route top 6]), both with the query's filter."""
    z, nodes, queries, qfilt = comp["z"], comp["nodes"], comp["queries"], comp["qfilt"]
    content_r = BM25Retriever.from_defaults(nodes=nodes, tokenizer=tokenizer, similarity_top_k=192, bm25_type=bm25_type)
    path_r = BM25Retriever.from_defaults(nodes=nodes, tokenizer=tokenizer, similarity_top_k=6, embed_type=5,
                                         bm25_type=bm25_type, engine=content_r.engine)
    try:
        cs = content_r.retrieve_batch(queries, filter_dicts=qfilt)
        ps = path_r.retrieve_batch(queries, filter_dicts=qfilt)
        for qn in range(len(queries)):
            flat = cs[qn] + ps[qn]
            fused = HybridRetriever.fusion([cs[qn], ps[qn]], topk=256)
            where = {id(nd): j for j, nd in enumerate(flat)}
            want = z[f"yaml_t{bm25_type}_pos"][qn]
            assert [where[id(g)] for g in fused] == want[want >= 0].tolist(), qn
    finally:
        path_r.close()
        content_r.close()
