"""Host side of the rows route (HipVectorStore.query_batch(rows=), QdrantRetriever.retrieve_batch(rows=) / score_nodes, rows_route_max,
filters over more distinct values than a class column holds): which engine entry a batch reaches and with which lists, on a stub engine that
records its calls (the one of test_filter_grammar.py plus dense_topk_rows).  No GPU."""
import numpy as np
import pytest

from easyrag_amd import _lib
from easyrag_amd import retrievers as R
from easyrag_amd.engine import RetrievalEngine
from easyrag_amd.schema import TextNode
from test_filter_grammar import FieldCondition, Filter, HasIdCondition, MatchAny, MatchValue, StubEngine


class RowsStub(StubEngine):
    """Records a rows call as ("rows", B, list_ptr, list_rows, list_of) after the engine's own CSR conversion; query b gets the first k rows
    of its list with descending scores."""

    def dense_topk_rows(self, q, k, lists, list_of=None, normalize_q=False, device_out=False, stream=None):
        B = q.shape[0]
        ptr, rows, lo = RetrievalEngine.lists_to_csr(lists, list_of, B)
        for l in range(len(ptr) - 1):
            r = rows[ptr[l]:ptr[l + 1]]
            assert np.all(np.diff(r) > 0), "a list that is not strictly ascending reached the engine"
        self.calls.append(("rows", B, ptr, rows, lo))
        ids, sc, ln = np.full((B, k), -1, np.int32), np.zeros((B, k)), np.zeros(B, np.int32)
        for b in range(B):
            r = rows[ptr[lo[b]]:ptr[lo[b] + 1]][:k] if lo[b] >= 0 else rows[:0]
            ids[b, :len(r)], ln[b] = r, len(r)
            sc[b, :len(r)] = 100.0 - np.arange(len(r))
        return ids, sc, ln


def _store(n=16, engine=None):
    eng = engine or RowsStub()
    dirs = ["a", "b", "c", "d"]
    nodes = [TextNode(text=f"t{i}", metadata={"dir": dirs[i % 4], "kind": "xy"[i % 2]}, id_=f"n{i}") for i in range(n)]
    return eng, R.HipVectorStore(nodes, np.eye(n, 64, dtype=np.float32), engine=eng)


def _lists(call):
    _, B, ptr, rows, lo = call
    return [list(rows[ptr[l]:ptr[l + 1]]) for l in range(len(ptr) - 1)], list(lo)


def test_rows_reach_the_rows_entry_sorted_unique_and_deduplicated():
    eng, store = _store()
    q = np.eye(5, 64, dtype=np.float32)
    shared = [9, 3, 3, 7]
    ids, sc, ln = store.query_batch(q, 3, rows=[shared, np.array([7, 3, 9]), shared, [2], []])
    assert len(eng.calls) == 1 and eng.calls[0][0] == "rows" and eng.calls[0][1] == 5
    lists, lo = _lists(eng.calls[0])
    assert lists == [[3, 7, 9], [2], []] and lo == [0, 0, 0, 1, 2]           # same object and equal content: one device list
    assert list(ln) == [3, 3, 3, 1, 0] and list(ids[3]) == [2, -1, -1]
    eng.calls.clear()
    store.query_batch(q, 3, rows=np.array([5, 1, 1]))                          # one array for every query
    lists, lo = _lists(eng.calls[0])
    assert lists == [[1, 5]] and lo == [0] * 5
    eng.calls.clear()
    store.query_batch(q[:3], 3, rows=[4, 2, 0])                                # a flat list of ids is ONE array, even of the batch's length
    lists, lo = _lists(eng.calls[0])
    assert lists == [[0, 2, 4]] and lo == [0, 0, 0]
    with pytest.raises(ValueError, match="rows must lie"):
        store.query_batch(q, 3, rows=[16])
    with pytest.raises(ValueError, match="rows must lie"):
        store.query_batch(q, 3, rows=[-1, 2])


def test_queries_without_rows_run_as_today_and_are_scattered():
    eng, store = _store()
    q = np.eye(4, 64, dtype=np.float32)
    ids, sc, ln = store.query_batch(q, 3, filters=[{"dir": "b"}, None, None, {"dir": "c"}], rows=[None, [8, 1], None, None])
    kinds = [c[0] for c in eng.calls]
    assert sorted(kinds) == ["column", "rows"]
    col = next(c for c in eng.calls if c[0] == "column")
    assert col[1] == 3 and list(col[2]) == [1, -1, 2]                          # today's call, today's column, for the three others
    lists, lo = _lists(next(c for c in eng.calls if c[0] == "rows"))
    assert lists == [[1, 8]] and lo == [0]
    assert list(ids[1]) == [1, 8, -1] and ln[1] == 2                           # the rows query's answer in its own row
    assert list(ids[0]) == [0, 1, 2] and list(ln) == [3, 2, 3, 3]              # (the stub's column answer)
    eng.calls.clear()
    store.query_batch(q, 3, filters=[{"dir": "b"}, None, None, {"dir": "c"}], rows=None)
    assert [c[0] for c in eng.calls] == ["column"] and list(eng.calls[0][2]) == [1, -1, -1, 2]
    eng.calls.clear()
    store.query_batch(q, 3, rows=[None] * 4)                                   # nobody carries rows: exactly today's call
    assert eng.calls == [("column", 4, None)]


def test_rows_with_a_filter_is_the_intersection():
    eng, store = _store()
    q = np.eye(5, 64, dtype=np.float32)
    r = np.arange(16)
    any_ac = Filter(must=[FieldCondition(key="dir", match=MatchAny(any=["a", "c"]))])
    nothing = Filter(must=[FieldCondition(key="dir", match=MatchAny(any=["zzz"]))])
    store.query_batch(q, 3, filters=[{"dir": "b"}, any_ac, nothing, {"dir": "zzz"}, None], rows=[r, [0, 1, 2, 3, 4, 6], r, r, [5]])
    assert [c[0] for c in eng.calls] == ["rows"]
    lists, lo = _lists(eng.calls[0])
    assert [lists[l] for l in lo] == [[1, 5, 9, 13], [0, 2, 4, 6], [], [], [5]]
    eng.calls.clear()
    kind_x_or_b = Filter(should=[FieldCondition(key="kind", match=MatchValue(value="x")), FieldCondition(key="dir", match=MatchValue(value="b"))])
    store.query_batch(q[:1], 3, filters=kind_x_or_b, rows=[[1, 2, 3, 4, 5]])      # a filter over two keys
    lists, lo = _lists(eng.calls[0])
    assert lists == [[1, 2, 4, 5]]                                             # kind x: even rows; dir b: 1, 5


def test_fast_mode_with_rows_raises_and_has_id_condition_still_does():
    eng, store = _store()
    q = np.eye(2, 64, dtype=np.float32)
    with pytest.raises(ValueError, match="ERH_DENSE_EXACT"):
        store.query_batch(q, 3, mode=_lib.ERH_DENSE_FAST, rows=[1, 2])
    with pytest.raises(TypeError, match="HasIdCondition"):
        store.query_batch(q, 3, filters=Filter(must=[HasIdCondition(has_id=[1])]))
    with pytest.raises(TypeError, match="HasIdCondition"):
        store.query_batch(q, 3, filters=Filter(must=[HasIdCondition(has_id=[1])]), rows=[1, 2])
    assert eng.calls == []


def test_rows_route_max_is_opt_in():
    assert R.HipVectorStore.rows_route_max == 0
    eng, store = _store(n=18)                                                   # dirs a, b: 5 rows each; c, d: 4 rows each
    assert store.rows_route_max == 0
    q = np.eye(4, 64, dtype=np.float32)
    flt = [{"dir": "a"}, {"dir": "c"}, None, Filter(must=[FieldCondition(key="dir", match=MatchAny(any=["c", "d"]))])]
    store.query_batch(q, 3, filters=flt)
    assert [c[0] for c in eng.calls] == ["sets"]                                # default: today's routing
    eng.calls.clear()
    store.rows_route_max = 4
    store.query_batch(q, 3, filters=flt)
    kinds = sorted(c[0] for c in eng.calls)
    assert kinds == ["rows", "sets"]                                            # class c (4 rows) -> rows; a (5), unfiltered and c + d (8) stay
    lists, lo = _lists(next(c for c in eng.calls if c[0] == "rows"))
    assert lists == [[2, 6, 10, 14]] and lo == [0]
    kind, B, ptr, cls = next(c for c in eng.calls if c[0] == "sets")            # ... on today's entry for a batch with a set of two classes
    assert B == 3 and [list(cls[ptr[b]:ptr[b + 1]]) for b in range(3)] == [[0], [-1], [2, 3]]
    eng.calls.clear()
    store.rows_route_max = 8
    store.query_batch(q, 3, filters=flt)
    rows_call = next(c for c in eng.calls if c[0] == "rows")
    lists, lo = _lists(rows_call)
    assert [lists[l] for l in lo] == [[0, 4, 8, 12, 16], [2, 6, 10, 14], [2, 3, 6, 7, 10, 11, 14, 15]]
    other = [c for c in eng.calls if c[0] != "rows"]
    assert len(other) == 1 and other[0] == ("column", 1, None)                  # the unfiltered query alone
    eng.calls.clear()
    store.query_batch(q, 3, filters=flt, mode=_lib.ERH_DENSE_FAST)              # FAST ranks by the fp32 score: never routed to rows
    assert [c[0] for c in eng.calls] == ["sets"]


def test_rows_route_max_keeps_the_mixed_batch_on_todays_entries():
    eng, store = _store(n=18)
    store.rows_route_max = 4
    q = np.eye(3, 64, dtype=np.float32)
    store.query_batch(q, 3, filters=[{"dir": "a"}, {"dir": "c"}, {"dir": "zzz"}])
    col = next(c for c in eng.calls if c[0] == "column")
    assert col[1] == 2 and list(col[2]) == [0, 32767]                           # a large class and an unknown value: the column, as today


def _big_store():
    eng = RowsStub()
    n = 33000
    nodes = [TextNode(text=f"t{i}", metadata={"page": i, "dir": "ab"[i % 2]}, id_=f"n{i}") for i in range(n)]   # 33000 distinct pages > 32000
    return eng, nodes, R.HipVectorStore(nodes, np.zeros((n, 64), np.float32), engine=eng)


def test_more_than_32000_distinct_values_dense_goes_through_rows_sparse_still_raises():
    eng, nodes, store = _big_store()
    q = np.eye(3, 64, dtype=np.float32)
    eq = {"page": 31999}
    anyf = Filter(must=[FieldCondition(key="page", match=MatchAny(any=[5, 32500, 40000]))])
    ids, sc, ln = store.query_batch(q, 3, filters=[eq, anyf, None])
    kinds = sorted(c[0] for c in eng.calls)
    assert kinds == ["column", "rows"]
    lists, lo = _lists(next(c for c in eng.calls if c[0] == "rows"))
    assert [lists[l] for l in lo] == [[31999], [5, 32500]]
    assert next(c for c in eng.calls if c[0] == "column") == ("column", 1, None)
    assert list(ids[0]) == [31999, -1, -1] and list(ln[:2]) == [1, 2]
    eng.calls.clear()
    store.query_batch(q[:1], 3, filters=Filter(must=[FieldCondition(key="page", match=MatchValue(value=7))]), rows=[[6, 7, 8]])
    assert _lists(eng.calls[0])[0] == [[7]]                                    # rows and such a filter: still the intersection
    eng.calls.clear()
    store.query_batch(q[:2], 3, filters={"dir": "b"})                          # a small key set on the same corpus: today's column
    assert eng.calls[0][0] == "column" and list(eng.calls[0][2]) == [1, 1]
    with pytest.raises(ValueError, match="too many distinct filter values"):
        store.corpus.filter_column([{"page": 3}])                              # what the sparse route calls
    with pytest.raises(ValueError, match="too many distinct filter values"):
        store.query_batch(q[:1], 3, filters={"page": 3}, mode=_lib.ERH_DENSE_FAST)   # FAST cannot take the rows entry


def test_retriever_rows_and_score_nodes():
    eng, store = _store()

    class Embed:
        def get_query_embedding(self, s):
            return np.eye(1, 64, dtype=np.float32)[0]
    ret = R.QdrantRetriever(store, Embed(), similarity_top_k=2)
    out = ret.retrieve_batch(["q0", "q1"], rows=[[9, 4], None])
    assert [g.node.node_id for g in out[0]] == ["n4", "n9"]
    assert sorted(c[0] for c in eng.calls) == ["column", "rows"]
    eng.calls.clear()
    got = ret.score_nodes("q", [store.nodes[11], 3, R.NodeWithScore(node=store.nodes[5], score=0.0), 3])
    lists, lo = _lists(eng.calls[0])
    assert lists == [[3, 5, 11]] and lo == [0] and eng.calls[0][1] == 1
    assert [g.node.node_id for g in got] == ["n3", "n5", "n11"] and got[0].score > got[1].score
    assert [g.node.node_id for g in ret.score_nodes("q", [11, 3, 5], top_k=2)] == ["n3", "n5"]
    assert ret.score_nodes("q", []) == []
    with pytest.raises(ValueError, match="not part of this store"):
        ret.score_nodes("q", [TextNode(text="other", metadata={}, id_="zz")])
    nodes, sims = store.query(np.eye(1, 64, dtype=np.float32)[0], 2, rows=[12, 1])
    assert [n.node_id for n in nodes] == ["n1", "n12"]


def test_score_nodes_over_more_nodes_than_one_list_holds():
    eng, store = _store(n=2000)
    eng.calls.clear()

    class Embed:
        def get_query_embedding(self, s):
            return np.eye(1, 64, dtype=np.float32)[0]
    ret = R.QdrantRetriever(store, Embed(), similarity_top_k=2)
    got = ret.score_nodes("q", range(1, 1801))
    assert len(got) == 1800 and len({g.node.node_id for g in got}) == 1800
    lists, lo = _lists(eng.calls[0])
    assert [len(l) for l in lists] == [768, 768, 264] and lo == [0, 1, 2]
    sc = [g.score for g in got]
    assert sc == sorted(sc, reverse=True)
