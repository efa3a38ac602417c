"""Corpus-sharded layout, host side: the index slicer, the numpy statement of the merge (the yardstick of the kernel tests,
held against hand cases here), the slice arithmetic and CorpusShards' exchange on two gloo ranks."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from _shard_yardstick import merge_batch, merge_one, merge_rrf_one, pack_rows, random_lists, row_bytes
from easyrag_amd import dist as erd
from easyrag_amd.index import BM25S, OKAPI, build_bm25_index, slice_bm25_index
from oracle import BM25Okapi, BM25SLucene


def _host_sum(idx, q_ids):
    """Per-document sum of the payloads in query-token order: what the scan kernel computes (tests/test_index_vs_oracle.py)."""
    acc = np.zeros(idx.n_docs, idx.payload.dtype)
    for t in q_ids:
        s, e = idx.indptr[t], idx.indptr[t + 1]
        acc[idx.doc_ids[s:e]] = acc[idx.doc_ids[s:e]] + idx.payload[s:e]
    return acc


def _bits(a):
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


@pytest.mark.parametrize("variant", [OKAPI, BM25S])
def test_slice_bm25_index_scores_its_documents_as_the_parent_does(variant):
    rng = np.random.default_rng(40 + variant)
    n, vocab = 3000, 400
    corpus = [[f"t{int(x)}" for x in rng.integers(0, vocab, size=rng.integers(1, 30))] for _ in range(n)]
    idx = build_bm25_index(corpus, variant)
    ora = BM25Okapi(corpus, k1=1.5, b=0.75, epsilon=0.25) if variant == OKAPI else BM25SLucene().index(corpus)
    queries = [[f"t{int(x)}" for x in rng.integers(0, vocab + 3, size=rng.integers(1, 10))] for _ in range(20)]
    parent = []
    for q in queries:                                        # the parent against the oracle, as test_index_vs_oracle.py does
        got = _host_sum(idx, idx.tokens_to_ids(q))
        assert np.array_equal(_bits(got), _bits(ora.get_scores(q)))
        parent.append(got)
    for world in (1, 2, 3, 8):
        slices = [(erd.corpus_shard_bounds(n, r, world), None) for r in range(world)]
        slices = [(b, slice_bm25_index(idx, *b)) for b, _ in slices]
        df = np.zeros(idx.n_vocab, np.int64)
        doc, tf, term, dl = [], [], [], []
        for (lo, hi), s in slices:
            assert s.n_docs == hi - lo and s.n_vocab == idx.n_vocab and s.variant == idx.variant
            assert s.idf is idx.idf and s.avgdl == idx.avgdl and s.average_idf == idx.average_idf and s.vocab is idx.vocab
            assert (s.k1, s.b, s.epsilon) == (idx.k1, idx.b, idx.epsilon)
            assert s.indptr.dtype == np.int64 and s.indptr[0] == 0 and s.indptr[-1] == s.nnz == s.doc_ids.shape[0]
            assert s.doc_ids.dtype == np.int32 and (s.nnz == 0 or (s.doc_ids.min() >= 0 and s.doc_ids.max() < hi - lo))
            assert s.payload.dtype == idx.payload.dtype and s.payload.shape[0] == s.nnz
            df += np.diff(s.indptr)
            doc.append(s.doc_ids.astype(np.int64) + lo)
            tf.append(s.tf)
            term.append(np.repeat(np.arange(idx.n_vocab), np.diff(s.indptr)))
            dl.append(s.doc_len)
        assert np.array_equal(df, np.diff(idx.indptr))
        assert np.array_equal(np.concatenate(dl), idx.doc_len)
        doc, tf, term = np.concatenate(doc), np.concatenate(tf), np.concatenate(term)
        order = np.lexsort((doc, term))                      # back into the parent's (term, document) order
        assert np.array_equal(doc[order], idx.doc_ids) and np.array_equal(tf[order], idx.tf)
        for qi, q in enumerate(queries):
            t = idx.tokens_to_ids(q)
            for (lo, hi), s in slices:
                assert np.array_equal(_bits(_host_sum(s, t)), _bits(parent[qi][lo:hi]))


def test_slice_bm25_index_without_payload_and_bad_ranges():
    rng = np.random.default_rng(3)
    corpus = [[f"t{int(x)}" for x in rng.integers(0, 20, size=rng.integers(1, 9))] for _ in range(50)]
    idx = build_bm25_index(corpus, OKAPI, compute_payload=False)
    s = slice_bm25_index(idx, 10, 25)
    assert s.payload.shape[0] == 0 and s.n_docs == 15 and np.array_equal(s.doc_len, idx.doc_len[10:25])
    for lo, hi in ((-1, 5), (5, 5), (40, 51)):
        with pytest.raises(ValueError):
            slice_bm25_index(idx, lo, hi)


def _lists(world, k, entries):
    """entries[r] = [(local id, score), ...] (canonical) -> the [world][k] arrays of one query."""
    ids = np.full((world, k), -1, np.int32)
    sc = np.zeros((world, k))
    ln = np.zeros(world, np.int32)
    for r, e in enumerate(entries):
        ln[r] = len(e)
        for i, (d, s) in enumerate(e):
            ids[r, i], sc[r, i] = d, s
    return ids, sc, ln


def test_numpy_merge_hand_cases():
    base = [0, 100, 200]
    # cross-rank ties: equal scores order by GLOBAL id, whichever rank they came from
    g, s = merge_one(*_lists(3, 4, [[(7, 2.0), (1, 1.0)], [(3, 2.0), (0, 1.0)], [(5, 3.0), (0, 2.0)]]), base, 4)
    assert g.tolist() == [205, 7, 103, 200] and s.tolist() == [3.0, 2.0, 2.0, 2.0]
    # a rank with an empty list
    g, s = merge_one(*_lists(3, 3, [[(2, 5.0)], [], [(9, 6.0), (1, 5.0)]]), base, 3)
    assert g.tolist() == [209, 2, 201] and s.tolist() == [6.0, 5.0, 5.0]
    # all ranks empty
    g, s = merge_one(*_lists(3, 3, [[], [], []]), base, 3)
    assert g.size == 0 and s.size == 0
    # sum(len) < k: everything, in order, no padding in the answer
    g, s = merge_one(*_lists(3, 8, [[(4, -1.0)], [(4, 0.5)], [(4, -1.0)]]), base, 8)
    assert g.tolist() == [104, 4, 204] and s.tolist() == [0.5, -1.0, -1.0]
    # batch form: padding is id -1 / score 0
    ids, sc, ln = _lists(3, 4, [[(4, -1.0)], [(4, 0.5)], []])
    o = merge_batch(ids[:, None], sc[:, None], ln[:, None], base, 4)
    assert o[0].tolist() == [[104, 4, -1, -1]] and o[1].tolist() == [[0.5, -1.0, 0.0, 0.0]] and o[2].tolist() == [2]


def test_numpy_merge_then_rrf_hand_cases():
    base = [0, 10]
    content = np.arange(20)
    content[12] = 3                                          # one content on two ranks: documents 3 (rank 0) and 12 (rank 1)
    sp = _lists(2, 3, [[(3, 9.0), (1, 2.0)], [(5, 4.0)]])    # global sparse list: 3, 15, 1
    dn = _lists(2, 3, [[(1, 0.9)], [(2, 0.95), (7, 0.5)]])   # global dense list: 12, 1, 17
    got = merge_rrf_one(sp, dn, base, 3, 3, content, K=1, topk=10)
    # content 3: 1/(1+1) (doc 3, sparse rank 1) + 1/(1+1) (doc 12, dense rank 1) = 1.0, node = the LAST seen = 12
    # content 1: 1/(3+1) + 1/(2+1); content 15: 1/3; content 17: 1/4
    assert got == [(12, 0.5 + 0.5), (1, 1 / 4 + 1 / 3), (15, 1 / 3), (17, 1 / 4)]
    assert merge_rrf_one(sp, dn, base, 3, 3, content, K=1, topk=1) == [(12, 1.0)]
    # an empty route, and everything empty
    e = _lists(2, 3, [[], []])
    assert merge_rrf_one(e, dn, base, 3, 3, content, K=60, topk=2) == [(12, 1 / 61), (1, 1 / 62)]
    assert merge_rrf_one(e, e, base, 3, 3, content, K=60, topk=2) == []
    # the cut of a route comes BEFORE the fusion: k_sparse = 1 keeps only document 3 of the sparse route
    assert [i for i, _ in merge_rrf_one(sp, dn, base, 1, 3, content, K=1, topk=10)] == [12, 1, 17]


def test_pack_rows_layout():
    rng = np.random.default_rng(1)
    for k in (1, 2, 5, 288):
        ids, sc, ln = random_lists(rng, 2, 3, k, slice_rows=1000)
        rows = pack_rows(ids, sc, ln)
        assert rows.shape == (2, 3, row_bytes(k)) and row_bytes(k) % 8 == 0 and row_bytes(k) >= 12 * k + 4
        host = erd._pack_rows_host(ids[1], sc[1], ln[1]).numpy()
        assert np.array_equal(host, rows[1])


def test_corpus_shard_bounds_cover_the_corpus():
    for n in (1, 7, 8, 1000, 30000, 8191):
        for w in (1, 2, 3, 8):
            if w > n:
                with pytest.raises(ValueError):
                    erd.CorpusShards(n, 0, w, engine=None)
                continue
            b = [erd.corpus_shard_bounds(n, r, w) for r in range(w)]
            assert b[0][0] == 0 and b[-1][1] == n and all(b[i][1] == b[i + 1][0] for i in range(w - 1))
            assert min(h - l for l, h in b) >= 1 and max(h - l for l, h in b) - min(h - l for l, h in b) <= 1
            cs = erd.CorpusShards(n, w - 1, w, engine=None)
            assert cs.mode == "host" and cs.bounds == b[-1] and cs.id_base.tolist() == [l for l, _ in b]
    with pytest.raises(ValueError):
        erd.CorpusShards(100, 0, 2, engine=None, mode="torch")       # the packed gathers need the library


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _canned(n_docs, world, B, k):
    rng = np.random.default_rng(77)
    rows = min(erd.corpus_shard_bounds(n_docs, r, world)[1] - erd.corpus_shard_bounds(n_docs, r, world)[0] for r in range(world))
    return random_lists(rng, world, B, k, slice_rows=rows, tie_levels=5)


def _worker(rank, world, port, n_docs, B, k, out_dir):
    torch.cuda.is_available = lambda: False                   # these ranks stand in for GPU ranks on the host
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    erd.init_from_env()
    ids, sc, ln = _canned(n_docs, world, B, k)
    cs = erd.CorpusShards(n_docs, rank, world, engine=None)
    assert cs.mode == "host" and cs.bounds == erd.corpus_shard_bounds(n_docs, rank, world)
    for _ in range(2):                                        # a second call reuses the object
        g = cs.merge_topk(torch.from_numpy(ids[rank]), torch.from_numpy(sc[rank]), torch.from_numpy(ln[rank]))
    assert cs.transport == "gloo"
    np.savez(os.path.join(out_dir, f"c{rank}.npz"), ids=g[0].numpy(), sc=g[1].numpy(), ln=g[2].numpy())
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_two_rank_corpus_shards_host_transport(tmp_path):
    n_docs, B, k = 1001, 23, 10
    port = _free_port()
    mp.spawn(_worker, args=(2, port, n_docs, B, k, str(tmp_path)), nprocs=2, join=True)
    ids, sc, ln = _canned(n_docs, 2, B, k)
    base = [erd.corpus_shard_bounds(n_docs, r, 2)[0] for r in range(2)]
    want = merge_batch(ids, sc, ln, base, k)
    for r in range(2):                                        # every rank holds the GLOBAL lists
        z = np.load(tmp_path / f"c{r}.npz")
        assert np.array_equal(z["ids"], want[0]) and np.array_equal(z["ln"], want[2])
        assert np.array_equal(z["sc"].view(np.uint64), want[1].view(np.uint64))


def test_corpus_shards_world1_host_is_a_merge_of_one_list():
    ids, sc, ln = _canned(50, 1, 9, 6)
    cs = erd.CorpusShards(50, 0, 1, engine=None)
    g = cs.merge_topk(torch.from_numpy(ids[0]), torch.from_numpy(sc[0]), torch.from_numpy(ln[0]))
    want = merge_batch(ids, sc, ln, [0], 6)
    assert cs.transport == "local" and all(np.array_equal(a.numpy(), b) for a, b in zip(g, want))


def test_native_mode_runs_as_torch_with_the_reason_recorded():
    class _NoEngine:                                           # never called: only the mode decision is under test
        device = 0
    cs = erd.CorpusShards(10, 0, 2, engine=_NoEngine(), mode="native")
    assert cs.mode == "torch" and "query-shard order" in cs.fallback_reason
