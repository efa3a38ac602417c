"""CPU: the oracle and the shim's host paths against answers produced by the REFERENCE's own glue code
(tests/golden/ref_glue*.{json,npz}, written by tests/golden/make_ref_glue_fixture.py): BM25Retriever.filter,
HybridRetriever.fusion / .reciprocal_rank_fusion / ._aretrieve, get_node_content, the BM25 corpus text and the query
tokenisation.  Nodes are compared by identity (list, position), scores by their float64 bits, and the scores the
reference writes into its input nodes as a side effect are checked too."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from _ref_glue import FILES, GOLDEN, bits, composition_texts, filter_scores, floats, fuse_cases, load, rrf_K
from easyrag_amd.retrievers import BM25Retriever, HybridRetriever, get_node_content, tokenize_and_remove_stopwords
from easyrag_amd.schema import NodeWithScore, TextNode
from oracle.retrievers import Item

REFERENCE = os.environ.get("EASYRAG_REFERENCE", "/root/reference")
GENERATOR = os.path.join(GOLDEN, "make_ref_glue_fixture.py")
HOST_MAX_ITEMS = HybridRetriever.fusion_device_min            # two-list inputs above this take the device branch


def test_fixture_is_what_the_reference_answers():
    """Staleness: regenerate from the reference checkout and require the committed bytes (literal tie orders only when
    numpy's version matches the one recorded)."""
    probe = os.path.join(REFERENCE, "src", "easyrag", "custom", "retrievers.py")
    if not os.access(probe, os.R_OK):
        pytest.skip(f"reference checkout not readable at {REFERENCE} (set EASYRAG_REFERENCE)")
    r = subprocess.run([sys.executable, GENERATOR, "--check"], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, EASYRAG_REFERENCE=REFERENCE))
    assert r.returncode == 0, r.stdout + r.stderr


def test_fixture_files_are_small():
    for name in FILES:
        assert os.path.getsize(os.path.join(GOLDEN, name)) <= 300 * 1024, name


# ---------------------------------------------------------------------------------------------------------------------
# BM25Retriever.filter
def _filter_runs():
    data, _, _ = load()
    for case in data["filter"]:
        for j, run in enumerate(case["runs"]):
            yield case, run


def _matches(meta, fd):
    return fd is None or all(k in meta and meta[k] == v for k, v in fd.items())


def test_oracle_filter_matches_reference():
    n_literal = 0
    for case, run in _filter_runs():
        sc = filter_scores(case)
        mask = None if run["filter_dict"] is None else np.array([_matches(m, run["filter_dict"]) for m in case["meta"]],
                                                                 dtype=bool)
        got = oracle.bm25_filter(sc, run["top_k"], mask)
        assert [i for i, _ in got] == run["canonical"], (case["name"], run["top_k"], run["filter_dict"])
        assert [s for _, s in got] == [float(sc[i]) for i in run["canonical"]]
        if not case["ties"]:
            assert [i for i, _ in oracle.bm25_filter(sc, run["top_k"], mask, tie="literal")] == run["literal"]
            n_literal += 1
    assert n_literal > 0


def _shim_filter(case, run):
    nodes = [TextNode(text=f"doc {i}", metadata=dict(m), id_=f"n{i}") for i, m in enumerate(case["meta"])]
    r = object.__new__(BM25Retriever)
    r._nodes, r._similarity_top_k, r.filter_dict = nodes, run["top_k"], run["filter_dict"]
    sc = filter_scores(case)
    got = r.filter(sc)
    pos = {id(n): i for i, n in enumerate(nodes)}
    return [pos[id(g.node)] for g in got], [g.score for g in got], sc


def test_shim_filter_matches_reference():
    for case, run in _filter_runs():
        ids, scores, sc = _shim_filter(case, run)
        assert ids == run["canonical"], (case["name"], run["top_k"], run["filter_dict"])
        assert all(type(s) is float for s in scores)
        assert bits(scores).tolist() == bits([float(sc[i]) for i in ids]).tolist()


def test_shim_filter_top_k_zero_checks_length_after_rejected_nodes():
    """similarity_top_k == 0: the reference tests the length after EVERY walked node; a rejected first node ends the walk
    with nothing, a kept first node leaves the test unmet and every positive passing node is returned."""
    data, _, _ = load()
    case = next(c for c in data["filter"] if c["name"] == "issue_top0")
    run = next(r for r in case["runs"] if r["top_k"] == 0 and r["filter_dict"] == {"dir": "a"})
    assert run["canonical"] == []
    assert _shim_filter(case, run)[0] == []
    run = next(r for r in case["runs"] if r["top_k"] == 0 and r["filter_dict"] is None)
    assert run["canonical"] == [0, 1, 2, 3, 4]
    assert _shim_filter(case, run)[0] == [0, 1, 2, 3, 4]


# ---------------------------------------------------------------------------------------------------------------------
# fusion / reciprocal_rank_fusion
def _split(cid, sc, lens):
    out, g = [], 0
    for ln in lens:
        out.append([(g + j, int(cid[g + j]), float(sc[g + j])) for j in range(ln)])
        g += ln
    return out


def test_oracle_fusion_matches_reference():
    for name, cid, sc, lens, modes in fuse_cases():
        lists = [[Item(p, c, s) for p, c, s in lst] for lst in _split(cid, sc, lens)]
        for m, (pos, osc, topk_len) in modes.items():
            K = rrf_K(m)
            for topk, n in topk_len.items():
                got = oracle.fusion(lists, topk) if K is None else oracle.reciprocal_rank_fusion(lists, K=K, topk=topk)
                assert [g.idx for g in got] == pos[:n].tolist(), (name, m, topk)
                assert bits([g.score for g in got]).tolist() == bits(osc[:n]).tolist(), (name, m, topk)


def _shim_fuse(cid, sc, lens, K, topk):
    lists = [[NodeWithScore(node=TextNode(text=f"c{c}", id_=f"i{p}"), score=s) for p, c, s in lst]
             for lst in _split(cid, sc, lens)]
    flat = [nd for lst in lists for nd in lst]
    where = {id(nd): j for j, nd in enumerate(flat)}
    got = HybridRetriever.fusion(lists, topk=topk) if K is None else \
        HybridRetriever.reciprocal_rank_fusion(lists, K=K, topk=topk)
    return [where[id(g)] for g in got], [g.score for g in got], [nd.score for nd in flat]


def expected_post(sc, pos, osc, rrf):
    """Every input node's score after the call, as the reference leaves it: the node returned for a content (RRF) holds the
    fused score -- also when topk cut it from the answer -- and every other node keeps its own."""
    post = np.asarray(sc, np.float64).copy()
    if rrf:
        post[pos] = osc
    return post


def check_fused(got_pos, got_sc, got_post, sc, pos, osc, n, rrf, what):
    assert got_pos == pos[:n].tolist(), what
    assert bits(got_sc).tolist() == bits(osc[:n]).tolist(), what
    assert bits(got_post).tolist() == bits(expected_post(sc, pos, osc, rrf)).tolist(), what


def test_shim_host_fusion_matches_reference():
    n_cases = 0
    for name, cid, sc, lens, modes in fuse_cases():
        if sum(lens) > HOST_MAX_ITEMS:
            continue                                        # device branch: tests/test_gpu_ref_glue.py
        n_cases += 1
        for m, (pos, osc, topk_len) in modes.items():
            for topk, n in topk_len.items():
                got = _shim_fuse(cid, sc, lens, rrf_K(m), topk)
                check_fused(*got, sc, pos, osc, n, rrf_K(m) is not None, (name, m, topk))
    assert n_cases >= 14


# ---------------------------------------------------------------------------------------------------------------------
# HybridRetriever._aretrieve: route selection, filter push-down, RRF
class _Child:
    """Stub route: a fresh copy of a canned list per call; records the filter attribute it held and the one passed."""

    def __init__(self, canned, attr):
        self.canned, self.attr = canned, attr
        self.seen, self.passed, self.returned = [], [], []
        self.filter_dict = self.filters = "<unset>"

    def retrieve_batch(self, queries, **kw):
        self.seen.append(getattr(self, self.attr))
        self.passed.append(kw[self.attr + "s" if self.attr == "filter_dict" else self.attr])
        self.returned.append([NodeWithScore(node=TextNode(text=f"c{c}"), score=s) for c, s in self.canned])
        return [self.returned[-1]]


def test_shim_aretrieve_matches_reference():
    data, _, _ = load()
    ar = data["aretrieve"]
    canned = {side: [(c, float.fromhex(s)) for c, s in ar[side]] for side in ("sparse", "dense")}
    for run in ar["runs"]:
        sp, de = _Child(canned["sparse"], "filter_dict"), _Child(canned["dense"], "filters")
        h = HybridRetriever(de, sp, retrieval_type=run["retrieval_type"], topk=run["topk"])
        h.filter_dict, h.filters = run["filter_dict"], run["filters"]
        got = h.retrieve_batch(["q"])[0]
        where = {id(nd): [side, j] for side, ch in (("sparse", sp), ("dense", de)) for lst in ch.returned
                 for j, nd in enumerate(lst)}
        assert [where[id(g)] + [float(g.score).hex()] for g in got] == run["out"], run
        assert sp.seen == run["sparse_seen"] and de.seen == run["dense_seen"], run
        assert sp.passed == run["sparse_seen"] and de.passed == run["dense_seen"], run


# ---------------------------------------------------------------------------------------------------------------------
# get_node_content, BM25 corpus text, query tokenisation
def _content_nodes():
    from easyrag_amd.schema import RelatedNodeInfo
    data, _, _ = load()
    specs = data["node_content"]["nodes"]
    nodes = [TextNode(text=s["text"], metadata=s["metadata"], id_=f"n{i}") for i, s in enumerate(specs)]
    for n, s in zip(nodes, specs):
        if s["previous"] is not None:
            n.relationships["2"] = RelatedNodeInfo(node_id=f"n{s['previous']}")
    return data["node_content"], nodes


def _cutter_and_stop():
    sys.path.insert(0, GOLDEN)
    try:
        from make_ref_fixture import CharCutter, load_stopwords
    finally:
        sys.path.remove(GOLDEN)
    return CharCutter(), load_stopwords(os.path.join(GOLDEN, "hit_stopwords.txt"))


def test_get_node_content_matches_reference():
    rec, nodes = _content_nodes()
    nodeid2idx = {n.node_id: i for i, n in enumerate(nodes)}
    for et in range(7):
        got = [get_node_content(NodeWithScore(node=n, score=1.0), et, nodes, nodeid2idx) for n in nodes]
        assert got == rec["content"][str(et)], et


def test_bm25_corpus_text_matches_reference():
    rec, nodes = _content_nodes()
    cutter, stop = _cutter_and_stop()
    for et in range(6):
        got = [tokenize_and_remove_stopwords(cutter, get_node_content(n, et), stop) for n in nodes]
        assert got == rec["bm25_corpus"][str(et)], et


def test_query_tokenisation_matches_reference():
    data, _, _ = load()
    cutter, stop = _cutter_and_stop()
    rows = []
    with open(os.path.join(GOLDEN, "question.jsonl"), encoding="utf-8") as f:
        for line in f:
            if line.strip():
                q = json.loads(line)
                rows.append([q["id"], tokenize_and_remove_stopwords(cutter, q["query"], stop)])
    blob = json.dumps(rows, ensure_ascii=False, sort_keys=True).encode("utf-8")
    assert len(rows) == data["tokenize"]["n"] == 103
    assert hashlib.sha256(blob).hexdigest() == data["tokenize"]["sha256"]


# ---------------------------------------------------------------------------------------------------------------------
# composition corpus: the oracle's routes under the reference's glue
def test_oracle_composition_matches_reference():
    data, _, z = load()
    comp = data["composition"]
    texts, meta, queries, qfilt = composition_texts()
    toks_c = [t.split(" ") for t in texts]
    toks_p = [m["know_path"].split(" ") for m in meta]
    routes = {0: (oracle.BM25Okapi(toks_c, 1.5, 0.75, 0.25), oracle.BM25Okapi(toks_p, 1.5, 0.75, 0.25)),
              1: (oracle.BM25SLucene(1.5, 0.75).index(toks_c), oracle.BM25SLucene(1.5, 0.75).index(toks_p))}
    key = {}
    cid = [key.setdefault(t, i) for i, t in enumerate(texts)]
    x16 = z["doc_emb_f16"]
    for qn, (q, fd) in enumerate(zip(queries, qfilt)):
        mask = None if fd is None else np.array([m["dir"] == fd["dir"] for m in meta])
        qt = q.split(" ")
        for bt in (0, 1):
            sc = routes[bt][0].get_scores(qt)
            full = z[f"filter_t{bt}_ids"][qn]
            full = full[full >= 0].tolist()
            for k, n in zip(comp["filter_ks"], z[f"filter_t{bt}_lens"][qn]):
                assert [i for i, _ in oracle.bm25_filter(sc, k, mask)] == full[:n], (qn, bt, k)
            c = oracle.bm25_filter(sc, 192, mask)
            p = oracle.bm25_filter(routes[bt][1].get_scores(qt), 6, mask)
            items = [Item(i, cid[i], s) for i, s in c] + [Item(i, cid[i], s) for i, s in p]
            fused = oracle.fusion([items[:len(c)], items[len(c):]], topk=256)
            want = z[f"yaml_t{bt}_pos"][qn]
            want = want[want >= 0].tolist()
            assert [items.index(g) if False else _pos_of(items, g) for g in fused] == want, (qn, bt)
        did, _ = oracle.dense_exact_topk(x16, oracle.to_f16_unit(z["query_emb_f32"][qn]), comp["k_dense"], mask)
        assert did.tolist() == z["dense_ids"][qn].tolist()
        ds = oracle.dense_exact_scores(x16, oracle.to_f16_unit(z["query_emb_f32"][qn]))
        sc = routes[0][0].get_scores(qt)
        sp = oracle.bm25_filter(sc, 192, mask)
        rrf = oracle.reciprocal_rank_fusion([[Item(i, cid[i], s) for i, s in sp],
                                             [Item(int(i), cid[int(i)], float(ds[i])) for i in did]], topk=comp["topk_rrf"])
        n = int(z["rrf_len"][qn])
        assert [w.idx for w in rrf] == z["rrf_ids"][qn, :n].tolist(), qn
        assert bits([w.score for w in rrf]).tolist() == bits(z["rrf_scores"][qn, :n]).tolist(), qn


def _pos_of(items, g):
    for j, it in enumerate(items):
        if it is g:
            return j
    raise AssertionError("fused item is not one of the inputs")
