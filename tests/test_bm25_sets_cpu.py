"""Host side of the sparse route's set filters (BM25Retriever.filters / retrieve_batch(filters=), HybridRetriever.retrieve_batch(sparse_filters=)):
the C entry is declared, bound and exported; which engine entry a batch reaches and with which class sets, on a stub engine that records its
calls (the one of test_bm25_rows_cpu.py plus bm25_topk_sets, the fused call and the dense sets entry's device outputs).  No GPU."""
import os

import numpy as np
import pytest

from conftest import WhitespaceTokenizer
from easyrag_amd import retrievers as R
from easyrag_amd.engine import RetrievalEngine
from easyrag_amd.schema import TextNode
from oracle import bm25_filter
from test_bm25_rows_cpu import Embed, SparseStub, _Dev, _ids, _lists
from test_filter_grammar import FieldCondition, Filter, MatchAny, MatchExcept, MatchText, MatchValue, Range

N = 16
DIRS = ["a", "b", "c", "d"]


def test_entry_is_declared_bound_and_exported():
    from easyrag_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "easyrag_hip.h")) as f:
        assert "int erh_bm25_topk_sets(erh_handle *h" in f.read()
    assert "erh_bm25_topk_sets" in _lib.SIGNATURES and len(_lib.SIGNATURES["erh_bm25_topk_sets"][1]) == 12
    assert hasattr(_lib.load(), "erh_bm25_topk_sets")
    assert {"bm25_sets_calls", "bm25_sets_subqueries", "bm25_sets_merge_launches"} <= set(RetrievalEngine.STAT_NAMES)


class SetsStub(SparseStub):
    """SparseStub + the sets entries and the fused call.  A sparse sets call is recorded as ("bm25_sets", B, set_ptr, set_cls, slot, device_out)
    after the engine's own CSR conversion; the fused call as ("hybrid", B, sparse column, dense column)."""

    def bm25_topk_sets(self, q_indptr, q_tok, k, sets, device_out=False, stream=None, slot=None):
        B = len(q_indptr) - 1
        ptr, cls = RetrievalEngine.sets_to_csr(sets, B)
        self.calls.append(("bm25_sets", B, ptr, cls, slot, device_out))
        out = np.tile(np.arange(k, dtype=np.int32), (B, 1)), 50.0 - np.tile(np.arange(k, dtype=np.float64), (B, 1)), np.full(B, k, np.int32)
        return tuple(_Dev(a) for a in out) if device_out else out

    def dense_topk_sets(self, q, k, sets, mode=0, normalize_q=False, device_out=False, stream=None):
        out = super().dense_topk_sets(q, k, sets, mode=mode)
        return tuple(_Dev(a) for a in out) if device_out else out

    def dense_check(self, stream=None):
        self.calls.append(("dense_check",))

    def hybrid_topk(self, q, q_indptr, q_tok, k_dense=288, k_sparse=192, K=60, topk=256, filter_dir=None, filter_dense=None, slot=None, **kw):
        B = len(q_indptr) - 1
        self.calls.append(("hybrid", B, None if filter_dir is None else list(filter_dir), None if filter_dense is None else list(filter_dense)))
        return np.tile(np.arange(topk, dtype=np.int32), (B, 1)), np.ones((B, topk)), np.full(B, topk, np.int32)


def _meta(i):
    return {"dir": DIRS[i % 4], "kind": "xy"[(i // 4) % 2], "year": 2018 + i % 4}


def _setup(k=3, kd=3, n=N):
    eng = SetsStub()
    nodes = [TextNode(text=f"w{i} common", metadata=_meta(i), id_=f"n{i}") for i in range(n)]
    sparse = R.BM25Retriever(nodes, WhitespaceTokenizer(), similarity_top_k=k, stopwords={""}, engine=eng, device_build=False)
    store = R.HipVectorStore(nodes, np.eye(n, 64, dtype=np.float32), engine=eng)
    dense = R.QdrantRetriever(store, Embed(), similarity_top_k=kd)
    eng.calls.clear()
    return eng, nodes, sparse, dense


def _dir(match):
    return FieldCondition(key="dir", match=match)


def _sets(call):
    ptr, cls = call[2], call[3]
    return [[int(c) for c in cls[ptr[b]:ptr[b + 1]]] for b in range(len(ptr) - 1)]


ANY_AC = Filter(must=[_dir(MatchAny(any=["a", "c"]))])


@pytest.mark.parametrize("flt,want", [
    (ANY_AC, [0, 2]),
    (Filter(must=[_dir(MatchExcept(except_=["a"]))]), [1, 2, 3]),
    (Filter(must_not=[_dir(MatchValue(value="d"))]), [0, 1, 2]),
    (Filter(must=[FieldCondition(key="year", range=Range(gte=2020))]), [2, 3]),
    (Filter(should=[_dir(MatchValue(value="a")), Filter(must=[_dir(MatchValue(value="c"))])]), [0, 2]),
])
def test_set_filters_reach_the_sets_entry_with_their_classes(flt, want):
    eng, nodes, sparse, _ = _setup()
    out = sparse.retrieve_batch(["common"] * 2, filters=flt)
    assert [c[0] for c in eng.calls] == ["bm25_sets"] and eng.calls[0][1] == 2 and eng.calls[0][4] == sparse._slot
    assert _sets(eng.calls[0]) == [want, want]
    assert _ids(out) == [["n0", "n1", "n2"]] * 2
    eng.calls.clear()
    sparse.filters = flt                                                       # the attribute applies to every query
    sparse.retrieve_batch(["common"])
    assert _sets(eng.calls[0]) == [want]


def test_every_class_one_class_and_no_class():
    eng, nodes, sparse, _ = _setup()
    sparse.retrieve_batch(["common"] * 2, filters=Filter(must=[_dir(MatchAny(any=["a", "b", "c", "d"]))]))
    assert [c[:2] for c in eng.calls] == [("bm25", 2)] and eng.calls[0][2] is None          # every class: the unfiltered call
    eng.calls.clear()
    sparse.retrieve_batch(["common"] * 2, filters=Filter(must=[_dir(MatchAny(any=["b"]))]))
    one = eng.calls[:]
    eng.calls.clear()
    sparse.retrieve_batch(["common"] * 2, filter_dicts={"dir": "b"})
    assert [c[0] for c in one] == ["bm25"] and list(one[0][2]) == list(eng.calls[0][2]) == [1, 1]     # one class: today's column, today's class
    eng.calls.clear()
    out = sparse.retrieve_batch(["common"] * 2, filters=Filter(must=[_dir(MatchAny(any=["zzz"]))]))
    assert eng.calls == [] and out == [[], []]                                 # no class: no engine call, empty lists
    out = sparse.retrieve_batch(["common"] * 4, filters=[ANY_AC, None, Filter(must=[_dir(MatchAny(any=["b"]))]),
                                                        Filter(must=[_dir(MatchAny(any=["zzz"]))])])
    assert [c[0] for c in eng.calls] == ["bm25_sets"]
    assert list(eng.calls[0][2]) == [0, 2, 3, 4, 4] and list(eng.calls[0][3]) == [0, 2, -1, 1]      # one call: a set, {-1}, one class, the empty set


def test_filter_dict_and_filters_is_the_intersection():
    eng, nodes, sparse, _ = _setup()
    abc = Filter(must=[_dir(MatchAny(any=["a", "b", "c"]))])
    sparse.retrieve_batch(["common"], filter_dicts={"kind": "x"}, filters=abc)
    assert [c[0] for c in eng.calls] == ["bm25_sets"]
    table = sparse._corpus_state._classes
    assert table.keys == ("dir", "kind")                                       # one column over the keys of both filters
    allowed = {i for i in range(N) if int(table.ids[i]) in _sets(eng.calls[0])[0]}
    assert allowed == {i for i in range(N) if _meta(i)["kind"] == "x" and _meta(i)["dir"] in "abc"} and len(allowed) == 6
    eng.calls.clear()
    sparse.retrieve_batch(["common"], filter_dicts={"dir": "a"}, filters=Filter(must=[FieldCondition(key="kind", match=MatchValue(value="y"))]))
    assert [c[0] for c in eng.calls] == ["bm25"] and list(eng.calls[0][2]) == [table.values[("a", "y")]]   # two equalities: one class
    eng.calls.clear()
    out = sparse.retrieve_batch(["common"], filter_dicts={"dir": "a"}, filters=Filter(must=[_dir(MatchValue(value="b"))]))
    assert eng.calls == [] and out == [[]]                                     # contradicting equalities: nothing, no call
    sparse.filter_dict, sparse.filters = {"dir": "c"}, ANY_AC                  # both attributes
    sparse.retrieve_batch(["common"])
    assert [c[0] for c in eng.calls] == ["bm25"] and list(eng.calls[0][2]) == [2]


def test_rows_and_a_set_filter_go_through_the_rows_entry():
    eng, nodes, sparse, _ = _setup()
    out = sparse.retrieve_batch(["common"] * 3, filters=[ANY_AC, ANY_AC, None], rows=[np.arange(N), None, [5, 6]])
    assert sorted(c[0] for c in eng.calls) == ["bm25_rows", "bm25_sets"]       # a query with rows never reaches the sets call
    lists, lo = _lists(next(c for c in eng.calls if c[0] == "bm25_rows"))
    assert [lists[l] for l in lo] == [[0, 2, 4, 6, 8, 10, 12, 14], [5, 6]]
    assert _sets(next(c for c in eng.calls if c[0] == "bm25_sets")) == [[0, 2]]
    assert _ids(out)[0] == ["n0", "n2", "n4"]


def test_mixed_key_sets_split():
    eng, nodes, sparse, _ = _setup()
    years = Filter(must=[FieldCondition(key="year", range=Range(lt=2020))])
    sparse.retrieve_batch(["common"] * 3, filters=[ANY_AC, years, None])
    assert [c[0] for c in eng.calls] == ["bm25_sets", "bm25_sets"]
    assert [c[1] for c in eng.calls] == [2, 1]                                 # the unfiltered query joins the first group
    assert _sets(eng.calls[0]) == [[0, 2], [-1]] and _sets(eng.calls[1]) == [[0, 1]]


def test_unsupported_elements_raise_before_any_engine_call():
    eng, nodes, sparse, dense = _setup()
    bad = Filter(must=[_dir(MatchText(text="a"))])
    with pytest.raises(TypeError, match="unsupported match"):
        sparse.retrieve_batch(["common"], filters=bad)
    with pytest.raises(TypeError, match="unsupported match"):
        R.HybridRetriever(dense, sparse, retrieval_type=3, topk=5).retrieve_batch(["common"], sparse_filters=bad)
    assert eng.calls == []


@pytest.mark.parametrize("k", [0, 1025])
def test_k_outside_the_device_range_takes_the_host_path_with_the_mask(k):
    eng, nodes, sparse, _ = _setup(k=k)
    eng.scores = np.array([3.0, 0.0, 5.0, 5.0, 1.0, -1.0, 2.0, 4.0, 0.5, 5.0, 0.0, 2.0, 7.0, 1.5, 6.0, 2.5])
    rows = [None, [12, 3, 9, 1, 5, 2, 14], None]
    fds = [None, None, {"kind": "y"}]
    out = sparse.retrieve_batch(["common"] * 3, filters=ANY_AC, filter_dicts=fds, rows=rows)
    assert [c[0] for c in eng.calls] == ["scores"] * 3                         # bm25_scores + the host walk, no device top-k
    for b in range(3):
        mask = np.array([_meta(i)["dir"] in "ac" for i in range(N)])
        if rows[b] is not None:
            keep = np.zeros(N, bool)
            keep[rows[b]] = True
            mask &= keep
        if fds[b]:
            mask &= np.array([_meta(i)["kind"] == "y" for i in range(N)])
        want = bm25_filter(eng.scores, k, mask)
        assert [(g.node.node_id, g.score) for g in out[b]] == [(f"n{i}", s) for i, s in want], b


def test_hybrid_without_sparse_filters_issues_todays_calls():
    eng, nodes, sparse, dense = _setup()
    hy = R.HybridRetriever(dense, sparse, retrieval_type=3, topk=3)
    q = ["common"] * 2
    hy.retrieve_batch(q, filter_dicts=[{"dir": "b"}, None], filters={"dir": "c"})
    assert eng.calls == [("hybrid", 2, [1, -1], [2, 2])]                       # an equality filter: the fused call, one column per route
    eng.calls.clear()
    hy.retrieve_batch(q, filter_dicts=[{"dir": "b"}, None], filters=ANY_AC)
    assert [c[0] for c in eng.calls] == ["bm25", "sets", "dense_check", "rrf", "sync"]     # a dense set filter: the column on the sparse route
    assert list(eng.calls[0][2]) == [1, -1] and list(eng.calls[1][3]) == [0, 2, 0, 2]
    eng.calls.clear()
    hy.retrieve_batch(q, filters=ANY_AC, sparse_filters=None)                  # None given: the same
    assert [c[0] for c in eng.calls] == ["bm25", "sets", "dense_check", "rrf", "sync"] and eng.calls[0][2] is None


def test_hybrid_with_sparse_filters_issues_sets_on_both_routes():
    eng, nodes, sparse, dense = _setup()
    hy = R.HybridRetriever(dense, sparse, retrieval_type=3, topk=3)
    q = ["common"] * 2
    out = hy.retrieve_batch(q, filters=ANY_AC, sparse_filters=ANY_AC)
    assert [c[0] for c in eng.calls] == ["bm25_sets", "sets", "dense_check", "rrf", "sync"]
    assert _sets(eng.calls[0]) == [[0, 2], [0, 2]] and eng.calls[0][5] is True and eng.calls[0][4] == sparse._slot
    assert list(eng.calls[1][3]) == [0, 2, 0, 2]
    assert _ids(out) == [["n0", "n1", "n2"]] * 2
    eng.calls.clear()
    hy.retrieve_batch(q, filter_dicts={"dir": "a"}, sparse_filters=ANY_AC)     # filter_dict AND the filter, dense unfiltered: still one pipeline
    assert [c[0] for c in eng.calls] == ["bm25_sets", "sets", "dense_check", "rrf", "sync"]
    assert _sets(eng.calls[0]) == [[0], [0]] and list(eng.calls[1][3]) == [-1, -1]
    eng.calls.clear()
    hy.retrieval_type = 2
    hy.retrieve_batch(q, sparse_filters=ANY_AC)                                # sparse only
    assert [c[0] for c in eng.calls] == ["bm25_sets"] and _sets(eng.calls[0]) == [[0, 2], [0, 2]]
    eng.calls.clear()
    hy.retrieval_type = 1
    hy.retrieve_batch(q, sparse_filters=ANY_AC)                                # dense only: the argument does not reach it
    assert eng.calls == [("column", 2, None)]


def test_more_than_32000_distinct_values_go_through_the_rows_entry():
    eng = SetsStub()
    n = 33000
    nodes = [TextNode(text=f"w{i % 50} common", metadata={"page": i, "dir": "ab"[i % 2]}, id_=f"n{i}") for i in range(n)]
    sparse = R.BM25Retriever(nodes, WhitespaceTokenizer(), similarity_top_k=3, stopwords={""}, engine=eng, device_build=False)
    eng.calls.clear()
    anyf = Filter(must=[FieldCondition(key="page", match=MatchAny(any=[5, 32500, 40000]))])
    out = sparse.retrieve_batch(["common"] * 3, filter_dicts=[{"page": 31999}, None, None], filters=[None, anyf, None])
    assert sorted(c[0] for c in eng.calls) == ["bm25", "bm25_rows"]            # nothing raises: the filtered queries as rows, the third as today
    lists, lo = _lists(next(c for c in eng.calls if c[0] == "bm25_rows"))
    assert [lists[l] for l in lo] == [[31999], [5, 32500]]
    assert _ids(out)[:2] == [["n31999"], ["n5", "n32500"]]
    eng.calls.clear()
    sparse.retrieve_batch(["common"], filter_dicts={"page": 7}, rows=[[6, 7, 8]])          # rows and such a filter: the intersection
    assert _lists(eng.calls[0])[0] == [[7]]
    eng.calls.clear()
    sparse.retrieve_batch(["common"] * 2, filter_dicts={"dir": "b"})           # a small key set on the same corpus: today's column
    assert [c[0] for c in eng.calls] == ["bm25"] and list(eng.calls[0][2]) == [1, 1]
    with pytest.raises(ValueError, match="too many distinct filter values"):
        sparse._corpus_state.filter_column([{"page": 3}])                      # the column itself keeps refusing
