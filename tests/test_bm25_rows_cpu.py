"""Host side of the sparse rows route (BM25Retriever.retrieve_batch(rows=) / score_nodes, HybridRetriever.retrieve_batch(sparse_rows=)):
which engine entry a batch reaches and with which lists, on a stub engine that records its calls (the one of test_dense_rows_cpu.py plus
the BM25 entries).  No GPU."""
import numpy as np
import pytest

from conftest import WhitespaceTokenizer
from easyrag_amd import retrievers as R
from easyrag_amd.engine import RetrievalEngine
from easyrag_amd.schema import TextNode
from oracle import bm25_filter
from test_dense_rows_cpu import RowsStub

N = 16
DIRS = ["a", "b", "c", "d"]


class _Dev:
    """What a device-output call hands back, as far as the retrievers touch it."""

    def __init__(self, a):
        self.a = np.asarray(a)

    def cpu(self):
        return self

    def numpy(self):
        return self.a


class SparseStub(RowsStub):
    """RowsStub + the BM25 entries.  A rows call is recorded as ("bm25_rows", B, list_ptr, list_rows, list_of, k, slot, device_out) after the
    engine's own CSR conversion, and query b gets the first k rows of its list with descending scores; the class-column call as
    ("bm25", B, column, slot) with the rows 0 .. k - 1."""

    def __init__(self):
        super().__init__()
        self.slots = 0
        self.scores = np.zeros(N)

    def alloc_bm25_slot(self):
        self.slots += 1
        return self.slots - 1

    def free_bm25_slot(self, slot):
        pass

    def set_bm25(self, index, payload_on_device=False, slot=None):
        pass

    def bm25_scores(self, q_tok, slot=None):
        self.calls.append(("scores", len(q_tok), slot))
        return self.scores.copy()

    def bm25_topk(self, q_indptr, q_tok, k, filter_dir=None, device_out=False, stream=None, slot=None):
        B = len(q_indptr) - 1
        self.calls.append(("bm25", B, None if filter_dir is None else np.array(filter_dir), slot))
        out = np.tile(np.arange(k, dtype=np.int32), (B, 1)), 50.0 - np.tile(np.arange(k, dtype=np.float64), (B, 1)), np.full(B, k, np.int32)
        return tuple(_Dev(a) for a in out) if device_out else out

    def bm25_topk_rows(self, q_indptr, q_tok, k, lists, list_of=None, device_out=False, stream=None, slot=None):
        B = len(q_indptr) - 1
        ptr, rows, lo = RetrievalEngine.lists_to_csr(lists, list_of, B)
        for l in range(len(ptr) - 1):
            assert np.all(np.diff(rows[ptr[l]:ptr[l + 1]]) > 0), "a list that is not strictly ascending reached the engine"
        self.calls.append(("bm25_rows", B, ptr, rows, lo, k, slot, device_out))
        ids, sc, ln = np.full((B, k), -1, np.int32), np.zeros((B, k)), np.zeros(B, np.int32)
        for b in range(B):
            r = rows[ptr[lo[b]]:ptr[lo[b] + 1]][:k] if lo[b] >= 0 else rows[:0]
            ids[b, :len(r)], ln[b] = r, len(r)
            sc[b, :len(r)] = 100.0 - np.arange(len(r))
        return tuple(_Dev(a) for a in (ids, sc, ln)) if device_out else (ids, sc, ln)

    def dense_topk_rows(self, q, k, lists, list_of=None, normalize_q=False, device_out=False, stream=None):
        out = super().dense_topk_rows(q, k, lists, list_of=list_of)
        return tuple(_Dev(a) for a in out) if device_out else out

    def rrf_device(self, ids_a, len_a, ids_b, len_b, K=60, topk=256, stream=None):
        self.calls.append(("rrf", ids_a.a.shape[0]))
        a, la = ids_a.a, len_a.a
        k = min(topk, a.shape[1])
        return _Dev(a[:, :k]), _Dev(np.ones((a.shape[0], k))), _Dev(np.minimum(la, k))

    def sync(self, stream=None):
        self.calls.append(("sync",))


class Embed:
    def get_query_embedding(self, s):
        return np.eye(1, 64, dtype=np.float32)[0]


def _setup(k=3, kd=3):
    eng = SparseStub()
    nodes = [TextNode(text=f"w{i} common", metadata={"dir": DIRS[i % 4], "kind": "xy"[i % 2]}, id_=f"n{i}") for i in range(N)]
    sparse = R.BM25Retriever(nodes, WhitespaceTokenizer(), similarity_top_k=k, stopwords={""}, engine=eng, device_build=False)
    store = R.HipVectorStore(nodes, np.eye(N, 64, dtype=np.float32), engine=eng)
    dense = R.QdrantRetriever(store, Embed(), similarity_top_k=kd)
    eng.calls.clear()
    return eng, nodes, sparse, dense


def _lists(call):
    ptr, rows, lo = call[2], call[3], call[4]
    return [list(rows[ptr[l]:ptr[l + 1]]) for l in range(len(ptr) - 1)], list(lo)


def _ids(out):
    return [[g.node.node_id for g in lst] for lst in out]


def test_rows_reach_the_rows_entry_sorted_unique_and_deduplicated():
    eng, nodes, sparse, _ = _setup()
    shared = [9, 3, 3, 7]
    out = sparse.retrieve_batch(["common"] * 5, rows=[shared, np.array([7, 3, 9]), shared, [2], []])
    assert [c[0] for c in eng.calls] == ["bm25_rows"] and eng.calls[0][1] == 5 and eng.calls[0][5] == 3 and eng.calls[0][6] == sparse._slot
    lists, lo = _lists(eng.calls[0])
    assert lists == [[3, 7, 9], [2], []] and lo == [0, 0, 0, 1, 2]           # same object and equal content: one device list
    assert _ids(out) == [["n3", "n7", "n9"]] * 3 + [["n2"], []]
    assert out[0][0].score == 100.0 and out[0][1].score == 99.0
    eng.calls.clear()
    sparse.retrieve_batch(["common"] * 5, rows=np.array([5, 1, 1]))            # one array for every query
    lists, lo = _lists(eng.calls[0])
    assert lists == [[1, 5]] and lo == [0] * 5
    eng.calls.clear()
    sparse.retrieve_batch(["common"] * 3, rows=[4, 2, 0])                      # a flat list of ids is ONE array, even of the batch's length
    lists, lo = _lists(eng.calls[0])
    assert lists == [[0, 2, 4]] and lo == [0, 0, 0]


def test_the_two_routes_share_one_normalisation():
    eng, nodes, sparse, dense = _setup()
    assert dense._vector_store._per_query_rows([3, 1, 1], 2)[0].tolist() == R._per_query_rows([3, 1, 1], 2, N)[0].tolist() == [1, 3]
    assert R.HipVectorStore._rows_lists([np.array([1, 2]), np.array([1, 2])])[1].tolist() == [0, 0]


def test_range_errors():
    eng, nodes, sparse, _ = _setup()
    with pytest.raises(ValueError, match="rows must lie"):
        sparse.retrieve_batch(["common"], rows=[N])
    with pytest.raises(ValueError, match="rows must lie"):
        sparse.retrieve_batch(["common"], rows=[-1, 2])
    with pytest.raises(ValueError, match="not part of this retriever"):
        sparse.score_nodes("common", [TextNode(text="other", metadata={}, id_="zz")])
    assert eng.calls == []


def test_rows_with_a_filter_dict_is_the_intersection():
    eng, nodes, sparse, _ = _setup()
    r = np.arange(N)
    sparse.retrieve_batch(["common"] * 4, filter_dicts=[{"dir": "b"}, {"dir": "zzz"}, None, {"dir": "c"}], rows=[r, r, [5], [0, 1, 2, 3, 4, 6]])
    assert [c[0] for c in eng.calls] == ["bm25_rows"]                          # a query with rows never reaches the class-column call
    lists, lo = _lists(eng.calls[0])
    assert [lists[l] for l in lo] == [[1, 5, 9, 13], [], [5], [2, 6]]
    eng.calls.clear()
    sparse.filter_dict = {"dir": "a"}                                          # the attribute applies to every query, rows or not
    sparse.retrieve_batch(["common"] * 2, rows=[[0, 1, 4, 5], None])
    kinds = sorted(c[0] for c in eng.calls)
    assert kinds == ["bm25", "bm25_rows"]
    assert _lists(next(c for c in eng.calls if c[0] == "bm25_rows"))[0] == [[0, 4]]
    assert list(next(c for c in eng.calls if c[0] == "bm25")[2]) == [0]


def test_queries_without_rows_run_todays_call_and_are_scattered():
    eng, nodes, sparse, _ = _setup()
    out = sparse.retrieve_batch(["common"] * 4, filter_dicts=[{"dir": "b"}, None, None, {"dir": "c"}], rows=[None, [8, 1], None, None])
    assert sorted(c[0] for c in eng.calls) == ["bm25", "bm25_rows"]
    col = next(c for c in eng.calls if c[0] == "bm25")
    assert col[1] == 3 and list(col[2]) == [1, -1, 2]                          # today's call, today's column, for the three others
    lists, lo = _lists(next(c for c in eng.calls if c[0] == "bm25_rows"))
    assert lists == [[1, 8]] and lo == [0]
    assert _ids(out) == [["n0", "n1", "n2"], ["n1", "n8"], ["n0", "n1", "n2"], ["n0", "n1", "n2"]]
    eng.calls.clear()
    sparse.retrieve_batch(["common"] * 4, filter_dicts=[{"dir": "b"}, None, None, {"dir": "c"}])
    assert [c[0] for c in eng.calls] == ["bm25"] and list(eng.calls[0][2]) == [1, -1, -1, 2]
    eng.calls.clear()
    sparse.retrieve_batch(["common"] * 4, rows=[None] * 4)                     # nobody carries rows: exactly today's call
    assert [c[:2] for c in eng.calls] == [("bm25", 4)] and eng.calls[0][2] is None


@pytest.mark.parametrize("k", [0, 1100])
def test_k_outside_the_device_range_takes_the_host_path(k):
    eng, nodes, sparse, _ = _setup(k=k)
    eng.scores = np.array([3.0, 0.0, 5.0, 5.0, 1.0, -1.0, 2.0, 4.0, 0.5, 5.0, 0.0, 2.0, 7.0, 1.5, 6.0, 2.5])
    rows = [[12, 3, 9, 1, 5, 2], None, [14, 6, 2, 10]]
    fds = [None, {"dir": "c"}, {"dir": "c"}]
    out = sparse.retrieve_batch(["common"] * 3, filter_dicts=fds, rows=rows)
    assert [c[0] for c in eng.calls] == ["scores"] * 3                         # bm25_scores + the host walk, no device top-k
    dirs = np.array([DIRS[i % 4] for i in range(N)])
    for b in range(3):
        mask = np.ones(N, bool)
        if rows[b] is not None:
            mask[:] = False
            mask[rows[b]] = True
        if fds[b]:
            mask &= dirs == fds[b]["dir"]
        want = bm25_filter(eng.scores, k, mask)            # (k = 0: the reference's length check after every walked node, restated there)
        assert [(g.node.node_id, g.score) for g in out[b]] == [(f"n{i}", s) for i, s in want], b


def test_score_nodes_ranks_the_given_nodes_by_the_corpus_index():
    eng, nodes, sparse, _ = _setup()
    got = sparse.score_nodes("common", [nodes[11], 3, R.NodeWithScore(node=nodes[5], score=0.0), 3])
    assert [c[0] for c in eng.calls] == ["bm25_rows"] and eng.calls[0][1] == 1 and eng.calls[0][5] == 3
    lists, lo = _lists(eng.calls[0])
    assert lists == [[3, 5, 11]] and lo == [0]
    assert [g.node.node_id for g in got] == ["n3", "n5", "n11"] and got[0].score > got[1].score
    assert [g.node.node_id for g in sparse.score_nodes("common", [11, 3, 5], top_k=2)] == ["n3", "n5"]
    assert sparse.score_nodes("common", []) == []


def test_score_nodes_over_more_nodes_than_one_list_holds():
    eng = SparseStub()
    n = 2500
    nodes = [TextNode(text=f"w{i} common", metadata={}, id_=f"n{i}") for i in range(n)]
    sparse = R.BM25Retriever(nodes, WhitespaceTokenizer(), similarity_top_k=3, stopwords={""}, engine=eng, device_build=False)
    eng.calls.clear()
    got = sparse.score_nodes("common", range(1, 2201))
    lists, lo = _lists(eng.calls[0])
    assert [len(l) for l in lists] == [1024, 1024, 152] and lo == [0, 1, 2] and eng.calls[0][5] == 1024
    assert len(got) == 2200 and len({g.node.node_id for g in got}) == 2200
    sc = [g.score for g in got]
    assert sc == sorted(sc, reverse=True)


def test_hybrid_sparse_rows_and_rows_stay_on_their_own_routes():
    eng, nodes, sparse, dense = _setup()
    q = ["common"] * 3
    s_rows, d_rows = [[9, 1], [2], [4, 6, 8]], [[10, 11], [12], [13, 14, 15]]
    hy = R.HybridRetriever(dense, sparse, retrieval_type=2, topk=5)
    out = hy.retrieve_batch(q, rows=d_rows, sparse_rows=s_rows)                # type 2: sparse only, its rows go through
    assert [c[0] for c in eng.calls] == ["bm25_rows"] and _lists(eng.calls[0])[0] == [[1, 9], [2], [4, 6, 8]]
    assert _ids(out) == [["n1", "n9"], ["n2"], ["n4", "n6", "n8"]]
    eng.calls.clear()
    hy.retrieve_batch(q)                                                       # ... and without: today's call
    assert [c[0] for c in eng.calls] == ["bm25"]
    eng.calls.clear()
    hy.retrieval_type = 1
    hy.retrieve_batch(q, rows=d_rows, sparse_rows=s_rows)                      # type 1: dense only
    assert [c[0] for c in eng.calls] == ["rows"] and _lists(eng.calls[0])[0] == [[10, 11], [12], [13, 14, 15]]
    eng.calls.clear()
    hy.retrieval_type = 3
    hy.retrieve_batch(q, rows=d_rows, sparse_rows=s_rows)                      # type 3, lists on both routes: two device lists, RRF, one sync
    assert [c[0] for c in eng.calls] == ["bm25_rows", "rows", "rrf", "sync"]
    sp_call, de_call = eng.calls[0], eng.calls[1]
    assert _lists(sp_call)[0] == [[1, 9], [2], [4, 6, 8]] and sp_call[7] is True and sp_call[5] == 3
    assert _lists(de_call)[0] == [[10, 11], [12], [13, 14, 15]]               # sparse_rows never reached the dense call, nor rows the sparse one
    eng.calls.clear()
    same = [np.array([5, 1, 9])] * 3
    hy.retrieve_batch(q, rows=same, sparse_rows=same, filter_dicts=[{"dir": "b"}, None, None])
    assert [c[0] for c in eng.calls] == ["bm25_rows", "rows", "rrf", "sync"]
    assert [_lists(eng.calls[0])[0][l] for l in _lists(eng.calls[0])[1]] == [[1, 5, 9], [1, 5, 9], [1, 5, 9]]       # dir b: rows 1, 5, 9, 13
    assert _lists(eng.calls[1]) == ([[1, 5, 9]], [0, 0, 0])                   # filter_dict restricts the sparse route only
    eng.calls.clear()
    hy.retrieve_batch(q, rows=d_rows)                                          # rows alone keeps its meaning: today's composition
    assert [c[0] for c in eng.calls] == ["bm25", "rows", "rrf", "sync"]


def test_hybrid_mixed_batch_runs_the_routes_on_their_own():
    eng, nodes, sparse, dense = _setup()
    hy = R.HybridRetriever(dense, sparse, retrieval_type=3, topk=5)
    q = ["common"] * 3
    out = hy.retrieve_batch(q, rows=[[10, 11], [12], [13]], sparse_rows=[[9, 1], None, [4]])      # one query without sparse rows
    kinds = [c[0] for c in eng.calls]
    assert sorted(kinds) == ["bm25", "bm25_rows", "rows"] and "rrf" not in kinds                  # host RRF over the routes' own results
    assert _lists(next(c for c in eng.calls if c[0] == "bm25_rows")) == ([[1, 9], [4]], [0, 1])
    assert next(c for c in eng.calls if c[0] == "bm25")[1] == 1
    assert set(_ids(out)[0]) == {"n1", "n9", "n10", "n11"}
    eng.calls.clear()
    hy.retrieve_batch(q, sparse_rows=[[9, 1], [2], [4]])                       # sparse rows only: the dense route runs as without rows
    assert sorted(c[0] for c in eng.calls) == ["bm25_rows", "column"]
    eng.calls.clear()
    hy.retrieve_batch(q, rows=[[10], None, [13]], sparse_rows=[[9, 1], [2], [4]])
    assert sorted(c[0] for c in eng.calls) == ["bm25_rows", "column", "rows"]
