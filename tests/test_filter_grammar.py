"""CPU: Qdrant-style set filters on the dense route (MatchAny, MatchExcept, Range, should, must_not, nesting).  The class sets the
retrievers compute over the class column equal a brute-force evaluation of the same filter on every node; a stub engine records which
entry point a batch reaches (dense_topk with today's int16 column, or dense_topk_sets with a class-set CSR) and that unsupported
elements fail before any engine call.  The Qdrant models are small stand-ins with Qdrant's field names."""
from dataclasses import dataclass, field
from typing import Any, List, Optional

import numpy as np
import pytest
from hypothesis import HealthCheck, given, settings
from hypothesis import strategies as st

from easyrag_amd import retrievers as R
from easyrag_amd.engine import RetrievalEngine
from easyrag_amd.schema import TextNode


# ---- stand-ins for qdrant_client.models -------------------------------------------------------------------------------------------
@dataclass
class MatchValue:
    value: Any


@dataclass
class MatchAny:
    any: List[Any]


@dataclass
class MatchExcept:
    except_: List[Any]


@dataclass
class MatchText:
    text: str


@dataclass
class Range:
    gt: Optional[float] = None
    gte: Optional[float] = None
    lt: Optional[float] = None
    lte: Optional[float] = None


@dataclass
class FieldCondition:
    key: str
    match: Any = None
    range: Any = None
    geo_bounding_box: Any = None
    geo_radius: Any = None
    geo_polygon: Any = None
    values_count: Any = None
    is_empty: Any = None
    is_null: Any = None


@dataclass
class Filter:
    should: Any = None
    min_should: Any = None
    must: Any = None
    must_not: Any = None


@dataclass
class HasIdCondition:
    has_id: List[Any] = field(default_factory=list)


@dataclass
class PayloadField:
    key: str


@dataclass
class IsEmptyCondition:
    is_empty: PayloadField


@dataclass
class IsNullCondition:
    is_null: PayloadField


# ---- brute force: the filter evaluated on one node's metadata, straight from the stand-in objects -------------------------------
def _brute(c, meta) -> bool:
    if isinstance(c, Filter):
        must, should, must_not = (list(x or []) for x in (c.must, c.should, c.must_not))
        return (all(_brute(x, meta) for x in must) and (not should or any(_brute(x, meta) for x in should))
                and not any(_brute(x, meta) for x in must_not))
    v = meta.get(c.key)
    if v is None:                                          # absent (or None): fails every condition on the key
        return False
    if c.range is not None:
        r = c.range
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            return False
        return ((r.gt is None or v > r.gt) and (r.gte is None or v >= r.gte) and (r.lt is None or v < r.lt)
                and (r.lte is None or v <= r.lte))
    m = c.match
    if isinstance(m, MatchValue):
        return v == m.value
    if isinstance(m, MatchAny):
        return v in m.any
    return v not in m.except_


class StubEngine:
    corpus = None

    def __init__(self):
        self.meta = []
        self.calls = []

    def set_doc_meta(self, n, cid, dir_id):
        self.meta.append(None if dir_id is None else np.array(dir_id))

    def set_dense(self, x, normalize=False):
        pass

    def dense_topk(self, q, k, filter_dir=None, mode=0):
        self.calls.append(("column", q.shape[0], None if filter_dir is None else np.array(filter_dir)))
        B = q.shape[0]
        return np.tile(np.arange(k, dtype=np.int32), (B, 1)), np.zeros((B, k)), np.full(B, k, np.int32)

    def dense_topk_sets(self, q, k, sets, mode=0, normalize_q=False, device_out=False, stream=None):
        ptr, cls = RetrievalEngine.sets_to_csr(sets, q.shape[0])
        self.calls.append(("sets", q.shape[0], ptr, cls))
        B = q.shape[0]
        return np.tile(np.arange(k, dtype=np.int32), (B, 1)), np.zeros((B, k)), np.full(B, k, np.int32)


KEYS = ("dir", "kind", "year")
VALUES = (0, 1, 2, 2.5, "a", "b", "c")


def _allowed_nodes(corpus, spec, n):
    """Node indices the retrievers let a query with this compiled filter see."""
    if spec is None:
        return set(range(n))
    if isinstance(spec, dict):
        c = corpus.filter_class(spec)
        return {i for i in range(n) if corpus._classes.ids[i] == c}
    cs = corpus.class_set(spec)
    if cs is None:
        return set(range(n))
    if not spec.keys:
        return set()
    return {i for i in range(n) if int(corpus._classes.ids[i]) in cs}


# ---- hypothesis: random nested filters over 2-3 keys -------------------------------------------------------------------------------
keys_st = st.sampled_from(KEYS[:3])
value_st = st.sampled_from(VALUES)
leaf_st = st.one_of(
    st.builds(lambda k, v: FieldCondition(key=k, match=MatchValue(value=v)), keys_st, value_st),
    st.builds(lambda k, vs: FieldCondition(key=k, match=MatchAny(any=vs)), keys_st, st.lists(value_st, max_size=3)),
    st.builds(lambda k, vs: FieldCondition(key=k, match=MatchExcept(except_=vs)), keys_st, st.lists(value_st, max_size=3)),
    st.builds(lambda k, gt, gte, lt, lte: FieldCondition(key=k, range=Range(gt=gt, gte=gte, lt=lt, lte=lte)), keys_st,
              *[st.one_of(st.none(), st.sampled_from((0, 1, 1.5, 2, 2.5))) for _ in range(4)]),
)
clause_st = lambda inner: st.one_of(st.none(), st.lists(inner, max_size=3))
filter_st = st.recursive(
    st.builds(lambda m, s, n: Filter(must=m, should=s, must_not=n), clause_st(leaf_st), clause_st(leaf_st), clause_st(leaf_st)),
    lambda inner: st.builds(lambda m, s, n: Filter(must=m, should=s, must_not=n), clause_st(st.one_of(leaf_st, inner)),
                            clause_st(st.one_of(leaf_st, inner)), clause_st(st.one_of(leaf_st, inner))),
    max_leaves=8)
meta_st = st.lists(st.fixed_dictionaries({}, optional={k: value_st for k in KEYS[:3]}), min_size=1, max_size=40)


@settings(max_examples=300, deadline=None, suppress_health_check=[HealthCheck.too_slow])
@given(metas=meta_st, flt=filter_st)
def test_class_sets_equal_brute_force(metas, flt):
    nodes = [TextNode(text=f"t{i}", metadata=m, id_=f"n{i}") for i, m in enumerate(metas)]
    corpus = R._FilteredCorpus(nodes, StubEngine())
    spec = R._filter_spec(flt)
    want = {i for i, m in enumerate(metas) if _brute(flt, m)}
    assert _allowed_nodes(corpus, spec, len(nodes)) == want


def test_class_set_per_element():
    metas = [{"dir": "a", "year": 2020}, {"dir": "b", "year": 2021}, {"dir": "c", "year": 2022.5}, {"dir": "a"}, {"year": 2020},
             {"dir": "b", "year": "x"}]
    nodes = [TextNode(text=f"t{i}", metadata=m, id_=f"n{i}") for i, m in enumerate(metas)]
    corpus = R._FilteredCorpus(nodes, StubEngine())
    n = len(nodes)

    def see(f):
        return sorted(_allowed_nodes(corpus, R._filter_spec(f), n))
    assert see(Filter(must=[FieldCondition(key="dir", match=MatchAny(any=["a", "c"]))])) == [0, 2, 3]
    assert see(Filter(must=[FieldCondition(key="dir", match=MatchExcept(except_=["a"]))])) == [1, 2, 5]     # key absent: fails
    assert see(Filter(must_not=[FieldCondition(key="dir", match=MatchValue(value="a"))])) == [1, 2, 4, 5]   # ... so must_not passes
    assert see(Filter(must=[FieldCondition(key="year", range=Range(gte=2021))])) == [1, 2]                  # "x" is no number
    assert see(Filter(should=[FieldCondition(key="dir", match=MatchValue(value="c")),
                              FieldCondition(key="year", range=Range(lt=2021))])) == [0, 2, 4]
    assert see(Filter(must=[Filter(should=[FieldCondition(key="dir", match=MatchValue(value="a"))])],
                      must_not=[FieldCondition(key="year", match=MatchValue(value=2020))])) == [3]
    assert see(Filter()) == list(range(n))                                                                  # empty: every row
    assert see(Filter(must=[FieldCondition(key="dir", match=MatchValue(value="a")),
                            FieldCondition(key="dir", match=MatchValue(value="b"))])) == []                # must: all of them


def test_except_attribute_alias():
    m = type("MatchExceptAlias", (), {})()
    setattr(m, "except", ["a"])
    spec = R._filter_spec(Filter(must=[FieldCondition(key="dir", match=m)]))
    assert isinstance(spec, R._SetFilter) and spec.node[1][0] == ("except", "dir", ("a",))


@pytest.mark.parametrize("bad,word", [
    (Filter(must=[HasIdCondition(has_id=[1])]), "HasIdCondition"),
    (Filter(must=[IsEmptyCondition(is_empty=PayloadField(key="dir"))]), "IsEmptyCondition"),
    (Filter(must_not=[IsNullCondition(is_null=PayloadField(key="dir"))]), "IsNullCondition"),
    (Filter(must=[FieldCondition(key="dir", match=MatchText(text="a"))]), "MatchText"),
    (Filter(should=[FieldCondition(key="dir", geo_radius={"center": 0})]), "geo_radius"),
    (Filter(must=[FieldCondition(key="dir", values_count={"gt": 1})]), "values_count"),
    (Filter(must=[FieldCondition(key="meta.dir", match=MatchValue(value="a"))]), "meta.dir"),
    (Filter(must=[FieldCondition(key="tags[]", match=MatchValue(value="a"))]), "tags[]"),
    (Filter(should=[FieldCondition(key="dir", match=MatchValue(value="a"))], min_should=1), "min_should"),
    (Filter(must=[FieldCondition(key="year", range=Range(gte="2020"))]), "Range"),
    (object(), "object"),
])
def test_unsupported_elements_raise_before_any_engine_call(bad, word):
    eng = StubEngine()
    nodes = [TextNode(text=f"t{i}", metadata={"dir": "ab"[i % 2]}, id_=f"n{i}") for i in range(6)]
    store = R.HipVectorStore(nodes, np.eye(6, 64, dtype=np.float32), engine=eng)
    n_meta = len(eng.meta)
    with pytest.raises(TypeError, match=word.replace("[", r"\[").replace(".", r"\.")):
        store.query_batch(np.eye(2, 64, dtype=np.float32), 3, filters=[None, bad])
    assert eng.calls == [] and len(eng.meta) == n_meta


# ---- which entry point a batch reaches -------------------------------------------------------------------------------------------
def _store():
    eng = StubEngine()
    dirs = ["a", "b", "c", "d"]
    nodes = [TextNode(text=f"t{i}", metadata={"dir": dirs[i % 4], "kind": "xy"[i % 2]}, id_=f"n{i}") for i in range(16)]
    return eng, R.HipVectorStore(nodes, np.eye(16, 64, dtype=np.float32), engine=eng)


def test_equality_filters_reach_dense_topk_with_todays_column():
    eng, store = _store()
    q = np.eye(4, 64, dtype=np.float32)
    store.query_batch(q, 3, filters=[{"dir": "b"}, None, Filter(must=[FieldCondition(key="dir", match=MatchValue(value="c"))]),
                                     {"dir": "zzz"}])
    assert len(eng.calls) == 1 and eng.calls[0][0] == "column" and list(eng.calls[0][2]) == [1, -1, 2, 32767]
    eng.calls.clear()
    store.query_batch(q, 3, filters=Filter(must=[FieldCondition(key="dir", match=MatchValue(value="d"))]))
    assert eng.calls[0][0] == "column" and list(eng.calls[0][2]) == [3, 3, 3, 3]
    eng.calls.clear()
    store.query_batch(q, 3)
    assert eng.calls == [("column", 4, None)]


def test_set_filters_reach_dense_topk_sets_with_the_expected_csr():
    eng, store = _store()
    q = np.eye(6, 64, dtype=np.float32)
    any_ac = Filter(must=[FieldCondition(key="dir", match=MatchAny(any=["a", "c"]))])
    not_b = Filter(must_not=[FieldCondition(key="dir", match=MatchValue(value="b"))])
    nothing = Filter(must=[FieldCondition(key="dir", match=MatchAny(any=["zzz"]))])
    every = Filter(should=[FieldCondition(key="dir", match=MatchExcept(except_=["zzz"]))])
    one = Filter(must=[FieldCondition(key="dir", match=MatchAny(any=["d", "zzz"]))])
    ids, sc, ln = store.query_batch(q, 3, filters=[any_ac, not_b, nothing, every, one, {"dir": "b"}])
    assert len(eng.calls) == 1
    kind, B, ptr, cls = eng.calls[0]
    assert kind == "sets" and B == 6
    sets = [list(cls[ptr[b]:ptr[b + 1]]) for b in range(B)]
    # empty -> [] (no scan), all classes -> unfiltered, one class -> that class, dicts as today
    assert sets == [[0, 2], [0, 2, 3], [], [-1], [3], [1]]
    eng.calls.clear()
    # only collapsed filters (empty / all / one class): today's column call, the empty query left out and answered with nothing
    ids, sc, ln = store.query_batch(q[:3], 3, filters=[nothing, every, one])
    assert eng.calls[0][0] == "column" and eng.calls[0][1] == 2 and list(eng.calls[0][2]) == [-1, 3]
    assert list(ln) == [0, 3, 3] and list(ids[0]) == [-1, -1, -1]
    eng.calls.clear()
    store.query_batch(q[:2], 3, filters=[nothing, nothing])
    assert eng.calls == []


def test_set_filters_over_other_keys_group_by_key_set():
    eng, store = _store()
    q = np.eye(4, 64, dtype=np.float32)
    kind_or = Filter(should=[FieldCondition(key="kind", match=MatchValue(value="x")),
                             FieldCondition(key="dir", match=MatchValue(value="b"))])
    store.query_batch(q, 3, filters=[{"dir": "a"}, kind_or, None,
                                     Filter(must=[FieldCondition(key="dir", match=MatchAny(any=["a", "b"]))])])
    assert [c[0] for c in eng.calls] == ["sets", "sets"]
    assert eng.calls[0][1] == 3 and eng.calls[1][1] == 1                    # {dir}: queries 0, 2, 3; {dir, kind}: query 1


def test_retrieve_batch_and_filters_attribute_accept_set_filters():
    eng, store = _store()

    class Embed:
        def get_query_embedding(self, s):
            return np.eye(1, 64, dtype=np.float32)[0]
    ret = R.QdrantRetriever(store, Embed(), similarity_top_k=2,
                            filters=Filter(must=[FieldCondition(key="dir", match=MatchAny(any=["a", "b"]))]))
    out = ret.retrieve("q")
    assert len(out) == 2 and eng.calls[-1][0] == "sets"
    res = ret.retrieve_batch(["q1", "q2"], filters=[None, Filter(must_not=[FieldCondition(key="dir", match=MatchValue(value="a"))])])
    assert len(res) == 2 and eng.calls[-1][0] == "sets"


def test_sets_to_csr():
    ptr, cls = RetrievalEngine.sets_to_csr([[3, 1], None, [], [32767]], 4)
    assert list(ptr) == [0, 2, 3, 3, 4] and list(cls) == [3, 1, -1, 32767] and cls.dtype == np.int16
    with pytest.raises(ValueError):
        RetrievalEngine.sets_to_csr([[1]], 2)
