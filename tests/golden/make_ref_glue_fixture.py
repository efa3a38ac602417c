"""Record what the reference's OWN retrieval glue answers, for tests/test_ref_glue_fixture.py (CPU) and
tests/test_gpu_ref_glue.py (GPU).  A CPU script; it always runs as its own process (pytest never imports it: the
placeholder llama_index / qdrant modules it installs would leak into other tests).

    python tests/golden/make_ref_glue_fixture.py            # write the fixture files
    python tests/golden/make_ref_glue_fixture.py --check    # exit 0 iff the committed files are what it would write

The reference checkout is found through EASYRAG_REFERENCE (default /root/reference).  Its two glue modules,
src/easyrag/pipeline/ingestion.py and src/easyrag/custom/retrievers.py, are imported as they are; every third-party
module their import lines name (llama_index, qdrant_client, bm25s, rank_bm25, nltk, and the reference's own
transformation / splitter / hierarchical modules) is replaced by a generic placeholder.  The only concrete stand-ins are
NodeWithScore (node, score, get_content() delegating to the node) and NodeRelationship.PREVIOUS.  Nothing the fixture
pins goes through a placeholder: BM25 and cosine arithmetic come from this repository's oracle (the libraries are not
available offline), the glue around them from the reference.

Tie order.  The reference's filter walks scores.argsort()[::-1], whose order among equal scores is implementation-defined.
Every filter call runs twice: on the plain ndarray (`literal`, recorded with numpy's version) and on an ndarray subclass
whose argsort() is np.lexsort((-index, score)), so that [::-1] walks score desc, index asc (`canonical`, the order this
repository documents).  The reference code stays untouched; only the array handed to it differs.

Output (deterministic: sorted keys, floats as float.hex(), no timestamps, every input stored in full):
  ref_glue.json          small cases: filter, fusion, RRF, _aretrieve, get_node_content, BM25 corpus text, tokenisation
  ref_glue_fusion.npz    fusion / RRF inputs and answers of 511 ... 2049 items
  ref_glue_corpus.npz    the composition corpus (tokens, fp16 unit embeddings, queries) and its expected answers
Large answers are stored once at full length; a run with a smaller k / topk is recorded as its length after the
generator has asserted that it is a prefix of the full answer.
"""
from __future__ import annotations

import ast
import asyncio
import hashlib
import importlib.util
import io
import json
import os
import sys
import types
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

OUT_JSON = os.path.join(HERE, "ref_glue.json")
OUT_FUSION = os.path.join(HERE, "ref_glue_fusion.npz")
OUT_CORPUS = os.path.join(HERE, "ref_glue_corpus.npz")
BIG = 10 ** 9                                   # "no cut": longer than any list here


# ---------------------------------------------------------------------------------------------------------------------
# placeholders for the reference's imports
class _Placeholder:
    """Any class the reference imports and does not need here: accepts every constructor call, has no behaviour."""

    def __init__(self, *args, **kwargs):
        pass


class _PlaceholderModule(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        cls = type(name, (_Placeholder,), {})
        setattr(self, name, cls)
        return cls


class StubNode:
    """A node as the glue reads it: .text, .metadata, .node_id, .relationships, get_content()."""

    def __init__(self, text, metadata=None, node_id=None, relationships=None):
        self.text = text
        self.metadata = dict(metadata or {})
        self.node_id = node_id
        self.relationships = dict(relationships or {})

    def get_content(self, *args, **kwargs):
        return self.text


class NodeWithScore:
    def __init__(self, node, score=None):
        self.node = node
        self.score = score

    def get_content(self, *args, **kwargs):
        return self.node.get_content()

    @property
    def metadata(self):
        return self.node.metadata


class NodeRelationship:
    PREVIOUS = "PREVIOUS"


class RelatedNodeInfo:
    def __init__(self, node_id):
        self.node_id = node_id


def _imported_modules(path, package):
    """Absolute names of every module the file's import statements name (relative ones resolved against `package`)."""
    names = set()
    for st in ast.walk(ast.parse(open(path, encoding="utf-8").read())):
        if isinstance(st, ast.Import):
            names.update(a.name for a in st.names)
        elif isinstance(st, ast.ImportFrom):
            if st.level:
                base = package.split(".")[:len(package.split(".")) - st.level + 1]
                names.add(".".join(base + ([st.module] if st.module else [])))
            else:                                                   # absolute import
                names.add(st.module)
    return names


def load_reference(ref_root):
    src = os.path.join(ref_root, "src", "easyrag")
    files = {"easyrag.pipeline.ingestion": os.path.join(src, "pipeline", "ingestion.py"),
             "easyrag.custom.retrievers": os.path.join(src, "custom", "retrievers.py")}
    for p in files.values():
        if not os.path.isfile(p):
            sys.exit(f"reference checkout not found: {p} is missing (set EASYRAG_REFERENCE to the EasyRAG checkout)")
    wanted = set()
    for name, p in files.items():
        wanted |= _imported_modules(p, name.rsplit(".", 1)[0])
    for pkg in ("easyrag", "easyrag.pipeline", "easyrag.custom"):
        m = types.ModuleType(pkg)
        m.__path__ = []
        sys.modules[pkg] = m
    for name in sorted(wanted):
        if name in files or name.split(".")[0] in sys.stdlib_module_names:
            continue
        parts = name.split(".")
        for i in range(1, len(parts) + 1):
            sub = ".".join(parts[:i])
            if sub not in sys.modules:
                mod = _PlaceholderModule(sub)
                mod.__path__ = []
                sys.modules[sub] = mod
    schema = sys.modules["llama_index.core.schema"]
    schema.NodeWithScore = NodeWithScore
    schema.NodeRelationship = NodeRelationship
    loaded = {}
    for name, p in files.items():
        spec = importlib.util.spec_from_file_location(name, p)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        loaded[name] = mod
    return loaded["easyrag.pipeline.ingestion"], loaded["easyrag.custom.retrievers"]


class CanonicalScores(np.ndarray):
    """argsort() = np.lexsort((-index, score)): reversed, it walks score desc, index asc."""

    def argsort(self, *args, **kwargs):
        s = self.view(np.ndarray)
        return np.lexsort((-np.arange(s.shape[0]), s))


def hx(v):
    return float(v).hex()


def hxs(a):
    return [hx(v) for v in a]


# ---------------------------------------------------------------------------------------------------------------------
# BM25Retriever.filter
def run_filter(R, nodes, scores, top_k, filter_dict, canonical):
    r = object.__new__(R.BM25Retriever)
    r._nodes, r._similarity_top_k, r.filter_dict = nodes, top_k, filter_dict
    got = r.filter(scores.view(CanonicalScores) if canonical else scores)
    pos = {id(n): i for i, n in enumerate(nodes)}
    out = [pos[id(g.node)] for g in got]
    for g, i in zip(got, out):
        assert type(g.score) is float and g.score == float(scores[i])
    return out


def has_ties(scores):
    p = scores[scores > 0]
    return bool(len(np.unique(p)) != len(p))


FILTER_META_VALUES = [1, 2, True, 1.0, "1", 0]
FILTER_DICTS = [None, {}, {"dir": "a"}, {"dir": "a", "num": 1}, {"dir": "zzz"}, {"num": 1}, {"num": 1.0},
                {"num": True}]


def filter_cases(R):
    rng = np.random.default_rng(20241220)
    vecs = {}
    s = rng.standard_normal(200) * 3.0
    s[rng.choice(200, 12, replace=False)] = 0.0
    vecs["random_f64"] = s
    t = np.array([9.0, 8.0] + [7.0] * 5 + [6.5] * 3 + [6.0, 5.0] + [4.0] * 5 + [3.0] * 3 + list(rng.uniform(0.1, 2.9, 20))
                 + [0.0, -1.0, -0.0])
    vecs["ties_3_5"] = t[rng.permutation(t.shape[0])]
    vecs["signed_zero"] = np.array([3.0, 0.0, -0.0, 2.0, -1.0, 1.0, 0.0, 2.0, -0.0, 5e-324, -5e-324, 0.5])
    vecs["all_nonpositive"] = np.array([0.0, -0.0, -2.0, -1e-300, 0.0, -3.5])
    f32 = rng.gamma(1.2, 2.0, 150).astype(np.float32)
    f32[rng.choice(150, 60, replace=False)] = 0.0
    f32[[3, 40, 77]] = f32[10]
    f32[[5, 6, 90, 91, 120]] = np.float32(1.25)
    vecs["bm25s_f32"] = f32
    vecs["issue_top0"] = np.array([5.0, 4.0, 3.0, 2.0, 1.0, 0.0])
    vecs["empty"] = np.zeros(0)
    cases = []
    for name in sorted(vecs):
        sc = vecs[name]
        n = sc.shape[0]
        meta = [{"dir": "a" if i % 2 else "b", "num": 1} for i in range(n)]
        if name != "issue_top0":
            meta = [{"dir": "abc"[(i * 7) % 3], "num": FILTER_META_VALUES[(i * 5) % len(FILTER_META_VALUES)]}
                    for i in range(n)]
        nodes = [StubNode(f"doc {i}", meta[i]) for i in range(n)]
        n_pos = int((sc > 0).sum())
        runs = []
        for top_k in sorted({0, 1, 6, 192, n_pos + 5}):
            for fd in FILTER_DICTS:
                rec = {"top_k": top_k, "filter_dict": fd,
                       "canonical": run_filter(R, nodes, sc, top_k, fd, True),
                       "literal": run_filter(R, nodes, sc, top_k, fd, False)}
                runs.append(rec)
        cases.append({"name": name, "dtype": str(sc.dtype), "scores": hxs(sc), "meta": meta, "ties": has_ties(sc),
                      "runs": runs})
    return cases


# ---------------------------------------------------------------------------------------------------------------------
# HybridRetriever.fusion / .reciprocal_rank_fusion
def make_lists(cids, scores, lens):
    lists, g = [], 0
    for ln in lens:
        lists.append([NodeWithScore(StubNode(f"c{cids[g + j]}"), float(scores[g + j])) for j in range(ln)])
        g += ln
    return lists


def run_fuse(R, cids, scores, lens, rrf, K, topk):
    lists = make_lists(cids, scores, lens)
    where = {}
    for li, lst in enumerate(lists):
        for pi, nd in enumerate(lst):
            where[id(nd)] = sum(lens[:li]) + pi
    got = (R.HybridRetriever.reciprocal_rank_fusion(lists, K=K, topk=topk) if rrf
           else R.HybridRetriever.fusion(lists, topk=topk))
    pos = [where[id(g)] for g in got]
    out_sc = [g.score for g in got]
    post = [nd.score for lst in lists for nd in lst]
    return pos, out_sc, post


TOPKS = (-1, 0, 1, "nd-1", "nd", "nd+1", 256)


def fuse_record(R, cids, scores, lens, rrf, K):
    """The full answer (topk = BIG), and per topk its length after asserting prefix and identical side effects."""
    pos, out_sc, post = run_fuse(R, cids, scores, lens, rrf, K, BIG)
    nd = len(set(int(c) for c in cids))
    assert len(pos) == nd
    lens_by_topk = {}
    for t in TOPKS:
        tk = t if isinstance(t, int) else nd + int(t[2:]) if len(t) > 2 else nd
        p2, s2, post2 = run_fuse(R, cids, scores, lens, rrf, K, tk)
        assert p2 == pos[:len(p2)] and all(x.hex() == y.hex() for x, y in zip(s2, out_sc))
        assert [x.hex() for x in post2] == [x.hex() for x in post]
        lens_by_topk[str(tk)] = len(p2)
    # side effects: every input node keeps its score, except the node returned for its content (RRF), which holds the
    # returned score -- checked here so that `post` need not be stored
    ret = dict(zip(pos, out_sc))
    for j, v in enumerate(post):
        want = ret[j] if (rrf and j in ret) else float(scores[j])
        assert v.hex() == want.hex()
    return pos, out_sc, lens_by_topk


def small_fuse_inputs():
    rng = np.random.default_rng(7)
    cases = []

    def add(name, lists_cs):
        lens = [len(l) for l in lists_cs]
        cids = [c for l in lists_cs for c, _ in l]
        scs = [s for l in lists_cs for _, s in l]
        cases.append((name, np.asarray(cids, np.int64), np.asarray(scs, np.float64), lens))

    add("dup_within", [[(1, 0.9), (2, 0.8), (1, 0.7), (3, 0.6), (1, 0.5)], [(4, 0.95), (2, 0.4)]])
    add("dup_across", [[(1, 3.0), (2, 2.0), (3, 1.0)], [(3, 5.0), (2, 4.0), (1, 0.5), (5, 0.25)]])
    add("all_one_content", [[(9, 1.0), (9, 2.0), (9, 3.0)], [(9, 4.0), (9, 0.5)]])
    add("first_empty", [[], [(1, 0.3), (2, 0.2), (1, 0.1)]])
    add("second_empty", [[(4, 0.3), (5, 0.2)], []])
    add("both_empty", [[], []])
    add("no_lists", [])
    add("single_list", [[(1, 0.3), (2, 0.3), (1, 0.2), (3, 0.1)]])
    add("three_lists", [[(1, 0.5), (2, 0.4)], [(2, 0.9), (3, 0.1), (1, 0.1)], [(4, 0.2), (3, 0.3), (2, 0.3)]])
    add("signed_scores", [[(1, 0.0), (2, -0.0), (3, -1.5), (4, 2.0), (5, 2.0)],
                          [(6, -0.0), (7, 0.0), (8, 2.0), (3, 7.0), (9, -1.5), (10, 5e-324)]])
    # symmetric ranks across lists: exact RRF ties, decided by first appearance
    add("rrf_rank_ties", [[(1, 0.9), (2, 0.8), (3, 0.7), (4, 0.6)], [(2, 0.9), (1, 0.8), (4, 0.7), (3, 0.6)]])
    a = [(int(c), float(s)) for c, s in zip(rng.integers(0, 30, 40), np.round(rng.uniform(-1, 1, 40), 2))]
    b = [(int(c), float(s)) for c, s in zip(rng.integers(0, 30, 33), np.round(rng.uniform(-1, 1, 33), 2))]
    add("random_73", [a, b])
    return cases


def big_fuse_inputs():
    rng = np.random.default_rng(2048)
    cases = []
    for n in (1, 511, 512, 513, 2047, 2048, 2049):
        na = n // 3 if n > 1 else 1
        pool = max(1, int(n * 0.7))
        cids = rng.integers(0, pool, n)
        sc = np.round(rng.uniform(-2.0, 6.0, n), 3)            # rounded: cross-list equal raw scores
        sc[rng.choice(n, max(1, n // 50), replace=False)] = 0.0
        sc[rng.choice(n, max(1, n // 50), replace=False)] = -0.0
        cases.append((f"items_{n}", cids.astype(np.int64), sc, [na, n - na]))
    return cases


def fusion_cases(R, arrays):
    out = []
    for big, inputs in ((False, small_fuse_inputs()), (True, big_fuse_inputs())):
        for name, cids, sc, lens in inputs:
            rec = {"name": name, "lens": lens, "n_distinct": len(set(int(c) for c in cids))}
            if big:
                arrays[f"{name}/cid"] = cids.astype(np.int32)
                arrays[f"{name}/score"] = sc
                rec["cid"] = rec["score"] = "npz"
            else:                                                   # small: inline
                rec["cid"] = [int(c) for c in cids]
                rec["score"] = hxs(sc)
            modes = [("fusion", False, 0)] + [(f"rrf_K{K}", True, K) for K in (0, 1, 60, 1000003)]
            for mname, rrf, K in modes:
                pos, osc, lens_t = fuse_record(R, cids, sc, lens, rrf, K)
                rec[mname] = {"topk_len": lens_t}
                if big:
                    arrays[f"{name}/{mname}/pos"] = np.asarray(pos, np.int32)
                    if rrf:
                        arrays[f"{name}/{mname}/score"] = np.asarray(osc, np.float64)
                    rec[mname]["pos"] = "npz"
                    rec[mname]["score"] = "npz" if rrf else "input"
                else:                                               # small: inline
                    rec[mname]["pos"] = pos
                    rec[mname]["score"] = hxs(osc) if rrf else "input"
            out.append(rec)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# HybridRetriever._aretrieve with stub children
class StubChild:
    """Returns a fresh copy of a canned list per call and records the filter attribute it held when called."""

    def __init__(self, canned, attr):
        self.canned, self.attr, self.seen, self.returned = canned, attr, [], []
        self.filter_dict = self.filters = "<unset>"

    async def aretrieve(self, query_bundle):
        self.seen.append(getattr(self, self.attr))
        self.returned.append([NodeWithScore(StubNode(f"c{c}"), s) for c, s in self.canned])
        return self.returned[-1]


ARETRIEVE_SPARSE = [(1, 12.5), (2, 9.0), (3, 9.0), (4, 1.0), (1, 0.5)]
ARETRIEVE_DENSE = [(3, 0.91), (5, 0.9), (1, 0.8), (6, 0.7), (2, 0.6), (7, 0.5), (5, 0.4)]


def aretrieve_cases(R):
    out = []
    for rt in (1, 2, 3):
        for topk in (6, 256):
            for fd, filt in ((None, None), ({"dir": "a"}, {"dir": "b"})):
                sp, de = StubChild(ARETRIEVE_SPARSE, "filter_dict"), StubChild(ARETRIEVE_DENSE, "filters")
                h = R.HybridRetriever(de, sp, retrieval_type=rt, topk=topk)
                h.filter_dict, h.filters = fd, filt
                got = asyncio.run(h._aretrieve(types.SimpleNamespace(query_str="q")))
                where = {id(nd): [side, j] for side, ch in (("sparse", sp), ("dense", de))
                         for lst in ch.returned for j, nd in enumerate(lst)}
                out.append({"retrieval_type": rt, "topk": topk, "filter_dict": fd, "filters": filt,
                            "sparse_seen": sp.seen, "dense_seen": de.seen,
                            "out": [where[id(g)] + [hx(g.score)] for g in got]})
    return out


# ---------------------------------------------------------------------------------------------------------------------
# get_node_content and the BM25 corpus text
NODE_SPECS = [
    # (text, metadata, previous node index or None)
    ("引言 段落\n图1 架构\n后文", {"file_path": "a/b.txt", "know_path": "K/一", "imgobjs": [
        {"cap": "图1", "title": "架构", "content": "三层结构"}]}, None),
    ("plain text only", {}, 0),
    ("说明\n| h1 | h2 | h3 |\n| --- | --- | --- |\n| x | y | z |", {"file_path": "t.md", "imgobjs": []}, 1),
    ("| 1 | 2 | 3 |\n| 4 | 5 | 6 |\n图2 流程\n", {"know_path": "K/二", "imgobjs": [
        {"cap": "图2", "title": "流程", "content": "步骤"}, {"cap": "图9", "title": "无", "content": "不用"}]}, 2),
    ("| 7 | 8 | 9 |\n| a | b | c |", {"file_path": "u.md"}, 1),
    ("| p | q |", {"know_path": "K/三"}, 2),
    ("| r | s | t | u | v |\n---\n", {}, 2),
    ("x | 4 | 5 |\n| 6 | 7 | 8 |", {"file_path": "v.md", "know_path": "K/四"}, 5),
    ("尾 | 1 | 2 | 3 |", {}, 3)]


def node_content_cases(ing, R, cutter, stop):
    nodes = [StubNode(t, m, f"n{i}") for i, (t, m, _) in enumerate(NODE_SPECS)]
    for node, (_, _, prev) in zip(nodes, NODE_SPECS):
        if prev is not None:
            node.relationships[NodeRelationship.PREVIOUS] = RelatedNodeInfo(f"n{prev}")
    nodeid2idx = {n.node_id: i for i, n in enumerate(nodes)}
    wrapped = [NodeWithScore(n, 1.0) for n in nodes]
    content = {str(et): [ing.get_node_content(w, et, nodes, nodeid2idx) for w in wrapped] for et in range(7)}
    corpus = {}
    for et in range(6):                         # the BM25 corpus of a retriever built with this embed_type
        r = R.BM25Retriever(wrapped, cutter, similarity_top_k=2, stopwords=stop, embed_type=et, bm25_type=0)
        corpus[str(et)] = r._corpus
    return {"nodes": [{"text": t, "metadata": m, "previous": p} for t, m, p in NODE_SPECS],
            "content": content, "bm25_corpus": corpus}


def token_record(R, cutter, stop):
    rows = []
    with open(os.path.join(HERE, "question.jsonl"), encoding="utf-8") as f:
        for line in f:
            if line.strip():
                q = json.loads(line)
                rows.append([q["id"], R.tokenize_and_remove_stopwords(cutter, q["query"], stop)])
    pinned = json.load(open(os.path.join(HERE, "ref_queries.json"), encoding="utf-8"))["queries"]
    assert [[p["id"], p["tokens"]] for p in pinned] == rows, "ref_queries.json differs from the reference tokenisation"
    blob = json.dumps(rows, ensure_ascii=False, sort_keys=True).encode("utf-8")
    return {"n": len(rows), "sha256": hashlib.sha256(blob).hexdigest()}


# ---------------------------------------------------------------------------------------------------------------------
# composition corpus: reference glue over oracle route arithmetic
N_DOCS, DIM, N_Q, VOCAB = 1500, 64, 48, 400
DIRS = ["umac", "rcp", "director", "emsplus"]
K_DENSE, TOPK_RRF = 288, 64
FILTER_KS = (0, 6, 192, 1100)
GAP = 1e-6


def composition(R, arrays):
    import oracle
    rng = np.random.default_rng(1500)
    p = 1.0 / np.arange(1, VOCAB + 1) ** 1.05
    p /= p.sum()
    docs = []
    for i in range(N_DOCS):
        if i > 10 and rng.random() < 0.02:
            docs.append(list(docs[int(rng.integers(0, i))]))        # duplicate content
        else:                                                       # fresh content
            docs.append([int(t) for t in rng.choice(VOCAB, int(rng.integers(3, 16)), p=p)])
    dir_id = rng.integers(0, len(DIRS), N_DOCS)
    kp_id = rng.integers(0, 12, N_DOCS)
    x16 = oracle.to_f16_unit(rng.standard_normal((N_DOCS, DIM)).astype(np.float32))
    texts = [" ".join(f"t{t}" for t in d) for d in docs]
    kps = [f"kp{k // 4} sec{k % 4}" for k in kp_id]
    nodes = [StubNode(texts[i], {"dir": DIRS[dir_id[i]], "know_path": kps[i]}, f"n{i}") for i in range(N_DOCS)]
    toks_c = [t.split(" ") for t in texts]
    toks_p = [k.split(" ") for k in kps]
    routes = {0: (oracle.BM25Okapi(toks_c, 1.5, 0.75, 0.25), oracle.BM25Okapi(toks_p, 1.5, 0.75, 0.25)),
              1: (oracle.BM25SLucene(1.5, 0.75).index(toks_c), oracle.BM25SLucene(1.5, 0.75).index(toks_p))}
    q_tok, q_emb, q_dir = [], [], []
    dense_ids = np.full((N_Q, K_DENSE), -1, np.int32)
    for qn in range(N_Q):
        ln = int(rng.integers(1, 6))
        qt = [int(t) for t in rng.integers(40, VOCAB, ln)]
        words = [f"t{t}" for t in qt]
        if qn % 3 == 0:
            words.append(f"kp{int(rng.integers(0, 3))}")
        qd = -1 if qn % 4 == 3 else int(rng.integers(0, len(DIRS)))
        mask = None if qd < 0 else dir_id == qd
        while True:                                    # a query embedding whose dense ranking no rounding can flip
            q32 = rng.standard_normal(DIM).astype(np.float32)
            s = oracle.dense_exact_scores(x16, oracle.to_f16_unit(q32))
            idx = np.arange(N_DOCS) if mask is None else np.nonzero(mask)[0]
            order = idx[np.lexsort((idx, -s[idx]))][:K_DENSE + 1]
            if np.all(np.diff(-s[order]) >= GAP):
                break                                  # every neighbour in the ranking at least GAP apart
        dense_ids[qn] = order[:K_DENSE]
        q_tok.append(words)
        q_emb.append(q32)
        q_dir.append(qd)
    arrays["doc_tok_flat"] = np.asarray([t for d in docs for t in d], np.int16)
    arrays["doc_tok_len"] = np.asarray([len(d) for d in docs], np.int16)
    arrays["doc_dir"] = dir_id.astype(np.int8)
    arrays["doc_kp"] = kp_id.astype(np.int8)
    arrays["doc_emb_f16"] = x16
    arrays["query_emb_f32"] = np.asarray(q_emb, np.float32)
    arrays["query_dir"] = np.asarray(q_dir, np.int8)
    arrays["dense_ids"] = dense_ids
    # BM25Retriever.filter over the oracle's route scores, per bm25_type; full answer at k = 1100 plus per-k lengths
    sparse_lists = {}
    for bt in (0, 1):
        full_ids = []
        lens = np.zeros((N_Q, len(FILTER_KS)), np.int32)
        for qn in range(N_Q):
            sc = routes[bt][0].get_scores(q_tok[qn])
            fd = None if q_dir[qn] < 0 else {"dir": DIRS[q_dir[qn]]}
            full = run_filter(R, nodes, sc, FILTER_KS[-1], fd, True)
            assert len(full) < FILTER_KS[-1] and len(full) == len(run_filter(R, nodes, sc, BIG, fd, True))
            for j, k in enumerate(FILTER_KS):
                got = run_filter(R, nodes, sc, k, fd, True)
                assert got == full[:len(got)] and (k == 0 or len(got) == min(k, len(full)))
                lens[qn, j] = len(got)
            full_ids.append(full)
            sparse_lists[(bt, qn)] = (sc, full)
        width = max(1, max(len(f) for f in full_ids))
        ids = np.full((N_Q, width), -1, np.int16)
        for qn, f in enumerate(full_ids):
            ids[qn, :len(f)] = f
        arrays[f"filter_t{bt}_ids"] = ids
        arrays[f"filter_t{bt}_lens"] = lens
    # _aretrieve types 1 / 2 / 3: sparse child = content route top 192 (bm25_type 0), dense child = the dense ranking
    rrf_ids = np.full((N_Q, TOPK_RRF), -1, np.int16)
    rrf_sc = np.zeros((N_Q, TOPK_RRF), np.float64)
    rrf_len = np.zeros(N_Q, np.int32)
    for qn in range(N_Q):
        sc, full = sparse_lists[(0, qn)]
        s_nodes = [(i, float(sc[i])) for i in full[:192]]
        ds = oracle.dense_exact_scores(x16, oracle.to_f16_unit(q_emb[qn]))
        d_nodes = [(int(i), float(ds[i])) for i in dense_ids[qn]]
        for rt in (1, 2, 3):
            sp = _ListChild(nodes, s_nodes)
            de = _ListChild(nodes, d_nodes)
            h = R.HybridRetriever(de, sp, retrieval_type=rt, topk=TOPK_RRF)
            got = asyncio.run(h._aretrieve(types.SimpleNamespace(query_str="q")))
            gi = [int(g.node.node_id[1:]) for g in got]
            if rt == 1:
                assert gi == [i for i, _ in d_nodes]
            elif rt == 2:
                assert gi == [i for i, _ in s_nodes]
            else:                                      # RRF of both routes
                rrf_ids[qn, :len(gi)] = gi
                rrf_sc[qn, :len(gi)] = [g.score for g in got]
                rrf_len[qn] = len(gi)
    arrays["rrf_ids"], arrays["rrf_scores"], arrays["rrf_len"] = rrf_ids, rrf_sc, rrf_len
    # the shipped yaml: fusion([content top 192 with the dir filter, know_path route top 6 with it]), per bm25_type
    for bt in (0, 1):
        pos = np.full((N_Q, 198), -1, np.int16)
        for qn in range(N_Q):
            fd = None if q_dir[qn] < 0 else {"dir": DIRS[q_dir[qn]]}
            c = run_filter(R, nodes, sparse_lists[(bt, qn)][0], 192, fd, True)
            pth = run_filter(R, nodes, routes[bt][1].get_scores(q_tok[qn]), 6, fd, True)
            assert len(c) + len(pth) <= 198
            csc, psc = sparse_lists[(bt, qn)][0], routes[bt][1].get_scores(q_tok[qn])
            lists = [[NodeWithScore(nodes[i], float(csc[i])) for i in c], [NodeWithScore(nodes[i], float(psc[i])) for i in pth]]
            where = {id(nd): j for j, nd in enumerate(lists[0] + lists[1])}
            got = R.HybridRetriever.fusion(lists, topk=256)
            pos[qn, :len(got)] = [where[id(g)] for g in got]
        arrays[f"yaml_t{bt}_pos"] = pos
    return {"n_docs": N_DOCS, "dim": DIM, "n_queries": N_Q, "dirs": DIRS, "k_dense": K_DENSE, "topk_rrf": TOPK_RRF,
            "filter_ks": list(FILTER_KS), "query_tokens": q_tok, "gap": GAP,
            "note": "doc text = ' '.join('t<id>'); know_path = 'kp<kp//4> sec<kp%4>'; queries are whitespace token lists"}


class _ListChild:
    def __init__(self, nodes, items):
        self.nodes, self.items = nodes, items
        self.filter_dict = self.filters = None

    async def aretrieve(self, query_bundle):
        return [NodeWithScore(self.nodes[i], s) for i, s in self.items]


# ---------------------------------------------------------------------------------------------------------------------
def npz_bytes(arrays):
    """np.savez_compressed without the wall-clock stamp: fixed zip dates, sorted names."""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            b = io.BytesIO()
            np.lib.format.write_array(b, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, b.getvalue())
    return buf.getvalue()


def build(ref_root):
    from make_ref_fixture import CharCutter, load_stopwords
    ing, R = load_reference(ref_root)
    cutter, stop = CharCutter(), load_stopwords(os.path.join(HERE, "hit_stopwords.txt"))
    fusion_arrays, corpus_arrays = {}, {}
    data = {
        "meta": {"numpy": np.__version__, "generator": "tests/golden/make_ref_glue_fixture.py",
                 "reference": "BUAADreamer/EasyRAG src/easyrag/{custom/retrievers.py,pipeline/ingestion.py}"},
        "filter": filter_cases(R),
        "fuse": fusion_cases(R, fusion_arrays),
        "aretrieve": {"sparse": [[c, hx(s)] for c, s in ARETRIEVE_SPARSE],
                      "dense": [[c, hx(s)] for c, s in ARETRIEVE_DENSE], "runs": aretrieve_cases(R)},
        "node_content": node_content_cases(ing, R, cutter, stop),
        "tokenize": token_record(R, cutter, stop),
        "composition": composition(R, corpus_arrays),
    }
    text = json.dumps(data, ensure_ascii=False, sort_keys=True, separators=(",", ":")) + "\n"
    return text.encode("utf-8"), npz_bytes(fusion_arrays), npz_bytes(corpus_arrays)


def _drop_literal(js):
    d = json.loads(js)
    for c in d["filter"]:
        for r in c["runs"]:
            r.pop("literal")
    d["meta"].pop("numpy")
    return d


def main(argv):
    ref = os.environ.get("EASYRAG_REFERENCE", "/root/reference")
    outs = dict(zip((OUT_JSON, OUT_FUSION, OUT_CORPUS), build(ref)))
    if "--check" in argv:
        bad = []
        for path, blob in outs.items():
            have = open(path, "rb").read() if os.path.exists(path) else b""
            if path == OUT_JSON and have:
                same_np = json.loads(have)["meta"]["numpy"] == np.__version__
                ok = have == blob if same_np else _drop_literal(have) == _drop_literal(blob)
            else:                                                   # .npz: bytes
                ok = have == blob
            if not ok:
                bad.append(os.path.basename(path))
        if bad:
            print("stale fixture files (rerun without --check): " + ", ".join(bad))
            return 1
        print("fixture files match the reference's answers")
        return 0
    for path, blob in outs.items():
        with open(path, "wb") as f:
            f.write(blob)
        print(f"wrote {path} ({len(blob)} bytes)")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
