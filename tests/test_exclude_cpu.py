"""Host side of the exclude lists (DESIGN K12): RetrievalEngine.excl_to_csr, the route rule plan_exclusion, the filter compiler's
HasIdCondition (must_not -> exclusion, must -> rows, anywhere else TypeError), which engine entry a batch with exclusions reaches (a stub
engine that records its calls: the one of test_dense_rows_cpu.py plus dense_topk_excl), and the two symbols in the header and the ctypes
table.  The Qdrant models are the stand-ins of test_filter_grammar.py.  No GPU."""
import re
from pathlib import Path

import numpy as np
import pytest

from easyrag_amd import _lib
from easyrag_amd import retrievers as R
from easyrag_amd.engine import RetrievalEngine
from easyrag_amd.schema import NodeWithScore
from test_dense_rows_cpu import RowsStub, _lists, _store
from test_filter_grammar import FieldCondition, Filter, HasIdCondition, MatchAny, MatchValue

ROOT = Path(__file__).resolve().parents[1]


def test_excl_to_csr_sorts_deduplicates_and_rejects():
    ptr, ids = RetrievalEngine.excl_to_csr([[9, 3, 3, 7], None, np.array([2]), [], (5, 4)], 5)
    assert ptr.dtype == np.int32 and ids.dtype == np.int32
    assert list(ptr) == [0, 3, 3, 4, 4, 6] and list(ids) == [3, 7, 9, 2, 4, 5]
    ptr, ids = RetrievalEngine.excl_to_csr(None, 3)                         # nothing excluded anywhere
    assert list(ptr) == [0, 0, 0, 0] and ids.shape == (0,)
    with pytest.raises(ValueError, match="one entry per query"):
        RetrievalEngine.excl_to_csr([[1]], 2)
    with pytest.raises(ValueError, match=r"\[0, 2\^31\)"):
        RetrievalEngine.excl_to_csr([[-1, 2]], 1)
    with pytest.raises(ValueError, match=r"\[0, 2\^31\)"):
        RetrievalEngine.excl_to_csr([[2 ** 31]], 1)
    with pytest.raises(ValueError, match="integers"):
        RetrievalEngine.excl_to_csr([[1.5]], 1)


def test_plan_exclusion_at_both_boundaries_of_each_route():
    for limit in (R.DENSE_MAX_K, R.BM25_DEVICE_MAX_K):
        assert R.plan_exclusion(1, 0, limit) == "drop"
        assert R.plan_exclusion(1, limit - 1, limit) == "drop" and R.plan_exclusion(1, limit, limit) == "complement"
        assert R.plan_exclusion(limit, 0, limit) == "drop" and R.plan_exclusion(limit, 1, limit) == "complement"
        assert R.plan_exclusion(288, limit - 288, limit) == "drop" and R.plan_exclusion(288, limit - 287, limit) == "complement"
    assert R.DENSE_MAX_K == 768 and R.BM25_DEVICE_MAX_K == 1024


def test_compiler_lifts_has_id_conditions():
    eng, store = _store()
    resolve = lambda e: R._id_positions(store, store.nodes, e, "store")
    dir_a = FieldCondition(key="dir", match=MatchValue(value="a"))
    f = Filter(must=[dir_a, HasIdCondition(has_id=[0, 4, 8, "n12"])], must_not=[HasIdCondition(has_id=["n4", 9]), HasIdCondition(has_id=[3])])
    rest, must_ids, not_ids = R._split_id_conditions(f)
    assert must_ids == [[0, 4, 8, "n12"]] and not_ids == ["n4", 9, 3]
    assert R._filter_spec(rest) == {"dir": "a"}                           # what is left is the payload filter, the equality shape here
    fl, rows, excl = R._lift_id_conditions(f, None, [[15]], 1, 16, resolve)
    assert list(rows[0]) == [0, 4, 8, 12] and list(excl[0]) == [3, 4, 9, 15]     # exclude= and must_not add up
    fl, rows, excl = R._lift_id_conditions([f, None], [[4, 8, 9], None], None, 2, 16, resolve)
    assert list(rows[0]) == [4, 8] and rows[1] is None and list(excl[0]) == [3, 4, 9] and excl[1].size == 0
    assert R._filter_spec(fl[0]) == {"dir": "a"} and fl[1] is None
    only = Filter(must_not=[HasIdCondition(has_id=[1])])
    fl, rows, excl = R._lift_id_conditions(only, None, None, 2, 16, resolve)
    assert rows is None and [list(e) for e in excl] == [[1], [1]] and R._filter_spec(fl[0]) is None
    plain = Filter(must=[dir_a])
    assert R._lift_id_conditions(plain, None, None, 2, 16, resolve) == (plain, None, None)   # no id condition: untouched
    # anywhere else: the compiler's TypeError, which says so
    for bad in (Filter(should=[HasIdCondition(has_id=[1])]), Filter(must=[Filter(must_not=[HasIdCondition(has_id=[1])])]),
                Filter(must_not=[Filter(must=[HasIdCondition(has_id=[1])])])):
        fl, _, _ = R._lift_id_conditions(bad, None, None, 1, 16, resolve)
        with pytest.raises(TypeError, match="HasIdCondition is served directly inside the top-level must"):
            R._filter_spec(fl[0] if isinstance(fl, list) else fl)
    with pytest.raises(ValueError, match="not part of this store"):
        resolve(["nope"])
    with pytest.raises(ValueError, match="positions must lie"):
        resolve([16])
    nws = NodeWithScore(node=store.nodes[5], score=1.0)
    assert list(resolve([nws, store.nodes[2], 5, "n7"])) == [2, 5, 7]


class ExclStub(RowsStub):
    def dense_topk_excl(self, q, k, exclude, sets=None, mode=0, normalize_q=False, device_out=False, stream=None):
        B = q.shape[0]
        eptr, eids = RetrievalEngine.excl_to_csr(exclude, B)
        self.calls.append(("excl", B, [list(eids[eptr[b]:eptr[b + 1]]) for b in range(B)],
                           None if sets is None else [None if s is None else list(s) for s in sets]))
        return np.tile(np.arange(k, dtype=np.int32), (B, 1)), np.zeros((B, k)), np.full(B, k, np.int32)


class _Embedder:
    def get_query_embedding(self, text):
        return np.eye(1, 64, dtype=np.float32)[0].tolist()


def test_which_entry_a_batch_with_exclusions_reaches():
    eng, store = _store(engine=ExclStub())
    r = R.QdrantRetriever(store, _Embedder(), similarity_top_k=3)
    r.retrieve_batch(["x", "y"], exclude=[[5, 1], None])
    assert eng.calls == [("excl", 2, [[1, 5], []], None)]
    eng.calls.clear()
    r.retrieve_batch(["x", "y"], exclude=[store.nodes[2], "n9"])            # one entry for every query
    assert eng.calls == [("excl", 2, [[2, 9], [2, 9]], None)]
    eng.calls.clear()
    any_ac = Filter(must=[FieldCondition(key="dir", match=MatchAny(any=["a", "c"]))], must_not=[HasIdCondition(has_id=[0])])
    r.retrieve_batch(["x", "y"], filters=[any_ac, {"dir": "b"}], exclude=[[4], [1]])
    assert eng.calls == [("excl", 2, [[0, 4], [1]], [[0, 2], [1]])]         # the payload filters as the call's class sets
    eng.calls.clear()
    r.retrieve_batch(["x"], rows=[[1, 2, 3, 4]], exclude=[[2, 9]])          # rows and an exclusion: a shorter list
    assert [c[0] for c in eng.calls] == ["rows"] and _lists(eng.calls[0])[0] == [[1, 3, 4]]
    eng.calls.clear()
    r.retrieve_batch(["x"], filters=Filter(must=[HasIdCondition(has_id=[1, 2, 3])], must_not=[HasIdCondition(has_id=[2])]))
    assert [c[0] for c in eng.calls] == ["rows"] and _lists(eng.calls[0])[0] == [[1, 3]]
    eng.calls.clear()
    r.retrieve_batch(["x", "y"], exclude=None)                              # nothing excluded: exactly today's call
    assert eng.calls == [("column", 2, None)]
    # too long for the drop route: the complement inside the allowed population, through the rows entry
    eng.calls.clear()
    keep, R.DENSE_MAX_K = R.DENSE_MAX_K, 5
    try:
        r.retrieve_batch(["x", "y"], filters=[{"dir": "a"}, None], exclude=[[0, 4, 5], [1]])
    finally:
        R.DENSE_MAX_K = keep
    kinds = sorted(c[0] for c in eng.calls)
    assert kinds == ["excl", "rows"]
    assert _lists(next(c for c in eng.calls if c[0] == "rows"))[0] == [[8, 12]]          # dir a = 0, 4, 8, 12 without 0, 4
    assert next(c for c in eng.calls if c[0] == "excl")[1:] == (1, [[1]], None)
    # the store itself takes positions only through exclude=, and its filters keep refusing id conditions
    with pytest.raises(TypeError, match="HasIdCondition"):
        store.query_batch(np.eye(1, 64, dtype=np.float32), 3, filters=Filter(must_not=[HasIdCondition(has_id=[1])]))


def test_symbols_in_header_and_ctypes_table():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "easyrag_hip.h").read_text(), flags=re.S)
    for name, n_args in (("erh_dense_topk_excl", 17), ("erh_bm25_topk_excl", 14)):
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n_args
    assert {"dense_excl_calls", "bm25_excl_calls", "excl_drop_launches"} <= set(RetrievalEngine.STAT_NAMES)
    from easyrag_amd import _build
    assert "exclude.hip" in _build.SOURCES
