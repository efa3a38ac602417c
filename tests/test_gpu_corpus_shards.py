"""Corpus-sharded layout on the GPU (easyrag_amd/csrc/shard_merge.hip, dist.CorpusShards): every slice of the corpus in a handle of
its own on the ONE device, run one after the other; the merged / fused result must equal the unsharded engine bit for bit.

  kernels   erh_shard_merge_topk / erh_shard_rrf through the C ABI against the numpy statement of tests/_shard_yardstick.py
            (held against hand cases in tests/test_corpus_shards_cpu.py)
  layout    the workload of tests/test_gpu_dist.py (30 000 x 256, 1003 queries) in both BM25 variants, world 1 / 3 / 8: dense
            EXACT, BM25 (k = 192, 1024), hybrid (-> 10, -> 256) against the unsharded calls and, on sampled queries, the oracle
  edges     slices shorter than k, duplicated rows in different slices, per-query dir filters, BM25 lists empty everywhere
  forms     one process with three handles; two processes on the one GPU through gloo (tests/_corpus_shard_rank_main.py)
  full size 1 M x 1024 + the 60 M-posting index in 4 slices

Dense FAST: its fp32 MFMA scores may depend on the tile a row lands in, and a slice places rows in other tiles than the whole
corpus does, so FAST lists are held to the rule of tests/test_gpu_dense.py (scores within 1e-3 of the exact ones, sorted), not
compared bit for bit."""
import numpy as np
import pytest

from _shard_yardstick import merge_batch, merge_rrf_one, pack_rows, random_lists
from easyrag_amd import _lib, dist as erd, synth
from easyrag_amd.engine import RetrievalEngine, queries_to_csr
from easyrag_amd.index import BM25S, OKAPI, build_bm25_index, build_bm25_index_from_ids, build_bm25_index_from_postings
from oracle import bm25_filter, dense_exact_scores, dense_exact_topk, reciprocal_rank_fusion
from oracle.retrievers import Item

pytestmark = pytest.mark.gpu


def _cpu(t):
    return tuple(a.cpu().numpy() for a in t)


def _same(got, want, what=""):
    """ids, fp64 score bits and lengths equal (padding included)."""
    assert np.array_equal(got[2], want[2]), f"{what}: lengths differ"
    assert np.array_equal(got[0], want[0]), f"{what}: ids differ"
    assert np.array_equal(np.ascontiguousarray(got[1]).view(np.uint64), np.ascontiguousarray(want[1]).view(np.uint64)), f"{what}: score bits differ"


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- the kernels through the C ABI ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("k", [1, 10, 192, 288, 768, 1024])
def test_shard_merge_kernel_equals_numpy_merge(engine, k, world):
    import torch
    rng = np.random.default_rng(1000 * world + k)
    B, rows = 9, 1500
    base = np.arange(world, dtype=np.int32) * rows
    cases = [dict(), dict(tie_levels=7), dict(tie_levels=3, empty_rank=world - 1)]     # random, equal fp64 bits across ranks, an empty rank
    for kw in cases:
        ids, sc, ln = random_lists(rng, world, B, k, rows, **kw)
        if "empty_rank" in kw:
            ln[:, 0] = 0                                                                # one query empty on every rank
        got = engine.shard_merge_topk(_dev(pack_rows(ids, sc, ln)), B, world, k, base)
        torch.cuda.synchronize()
        _same(_cpu(got), merge_batch(ids, sc, ln, base, k), f"k={k} world={world} {kw}")
    assert engine.topk_row_bytes(k) == pack_rows(ids, sc, ln).shape[2]


def test_shard_merge_reads_the_rows_erh_pack_topk_writes(engine):
    """The kernel's input is the library's own packed row, byte for byte what tests/_shard_yardstick.pack_rows states."""
    import torch
    rng = np.random.default_rng(5)
    world, B, k, rows = 3, 11, 37, 400                                                 # odd k: rows padded to 8 bytes
    ids, sc, ln = random_lists(rng, world, B, k, rows, tie_levels=4)
    recv = torch.empty((world, B, engine.topk_row_bytes(k)), dtype=torch.uint8, device="cuda")
    for r in range(world):
        engine.pack_topk(_dev(ids[r]), _dev(sc[r]), _dev(ln[r]), recv[r])
    torch.cuda.synchronize()
    assert np.array_equal(recv.cpu().numpy()[:, :, :12 * k + 4], pack_rows(ids, sc, ln)[:, :, :12 * k + 4])
    base = np.arange(world, dtype=np.int32) * rows
    got = engine.shard_merge_topk(recv, B, world, k, base)
    torch.cuda.synchronize()
    _same(_cpu(got), merge_batch(ids, sc, ln, base, k))


def test_shard_merge_of_short_lists_with_negative_scores(engine):
    """Three slices whose lists are all shorter than k and hold negative scores only (dense scores of a query that points away from the
    corpus): the padding entries of the packed rows carry (id -1, score 0.0), which would outrank every live entry if the merge took one for
    a row.  erh_pack_topk writes the rows; the merged lists (shorter than k too: padded again) equal the numpy merge."""
    import torch
    rng = np.random.default_rng(58)
    world, B, k, rows = 3, 13, 100, 700
    ids = np.full((world, B, k), -1, np.int32)
    sc = np.zeros((world, B, k), np.float64)
    ln = np.zeros((world, B), np.int32)
    levels = -(rng.random(5) + 0.25)
    for r in range(world):
        for q in range(B):
            n = int(rng.integers(0, 30)) if q else 0                                    # (query 0: empty on every rank)
            loc = rng.choice(rows, size=n, replace=False).astype(np.int64)
            s = levels[rng.integers(0, 5, size=n)] if q % 2 else -(rng.random(n) + 1e-3)   # equal bits across ranks / distinct scores
            order = np.lexsort((loc, -s))
            ids[r, q, :n], sc[r, q, :n], ln[r, q] = loc[order], s[order], n
    assert ln.sum(axis=0).max() < k and np.all(sc <= 0.0)
    recv = torch.empty((world, B, engine.topk_row_bytes(k)), dtype=torch.uint8, device="cuda")
    for r in range(world):
        engine.pack_topk(_dev(ids[r]), _dev(sc[r]), _dev(ln[r]), recv[r])
    base = np.arange(world, dtype=np.int32) * rows
    got = engine.shard_merge_topk(recv, B, world, k, base)
    torch.cuda.synchronize()
    got = _cpu(got)
    want = merge_batch(ids, sc, ln, base, k)
    _same(got, want)
    for q in range(B):
        assert got[2][q] == ln[:, q].sum() and np.all(got[0][q, :got[2][q]] >= 0) and np.all(got[1][q, :got[2][q]] < 0.0), q


@pytest.mark.parametrize("world", [1, 3, 8])
@pytest.mark.parametrize("k_sparse,k_dense", [(192, 288), (1024, 768), (1, 1), (1024, 10)])
def test_shard_rrf_kernel_equals_merge_then_oracle_rrf(engine, k_sparse, k_dense, world):
    import torch
    rng = np.random.default_rng(77 * world + k_sparse)
    B, rows = 5, 1300
    n = world * rows
    base = np.arange(world, dtype=np.int32) * rows
    content = np.arange(n, dtype=np.int32)
    dup = rng.choice(n, size=max(n // 100, 1), replace=False)                          # 1 % of the contents also live on another rank
    content[dup] = content[(dup + rows * rng.integers(1, max(world, 2), size=dup.shape[0])) % n]
    sp = random_lists(rng, world, B, k_sparse, rows, tie_levels=9)
    dn = random_lists(rng, world, B, k_dense, rows)
    for q in range(B):                                                                  # the routes overlap, as real retrieval does
        for r in range(world):
            m = min(sp[2][r, q], dn[2][r, q]) // 2
            keep = ~np.isin(dn[0][r, q, :dn[2][r, q]], sp[0][r, q, :m])
            if keep.all() and m:
                dn[0][r, q, :m] = sp[0][r, q, :m]
    sp[2][:, 0] = 0                                                                     # query 0: no sparse list anywhere
    engine.set_shard_content(content)
    try:
        rs, rd = _dev(pack_rows(*sp)), _dev(pack_rows(*dn))
        for K in (1, 60):
            for topk in (1, 10, 256, k_sparse + k_dense + 40):                          # the last: more than the distinct contents
                got = _cpu(engine.shard_rrf(rs, k_sparse, rd, k_dense, B, world, base, K=K, topk=topk))
                torch.cuda.synchronize()
                for q in range(B):
                    want = merge_rrf_one(tuple(a[:, q] for a in sp), tuple(a[:, q] for a in dn), base, k_sparse, k_dense, content, K, topk)
                    assert got[2][q] == len(want)
                    assert list(got[0][q, :len(want)]) == [i for i, _ in want], f"K={K} topk={topk} query {q}: ids differ"
                    assert list(got[1][q, :len(want)]) == [s for _, s in want], f"K={K} topk={topk} query {q}: scores differ"
                    assert np.all(got[0][q, len(want):] == -1) and np.all(got[1][q, len(want):] == 0)
    finally:
        engine.set_shard_content(None)


def test_shard_merge_limits(engine):
    """world * (12 k + 4) bytes must fit the 160 KiB of one CU: 13 x 1024 does (and is merged correctly), 14 x 1024 does not."""
    import torch
    rng = np.random.default_rng(3)
    world, k, B, rows = 13, 1024, 3, 1100
    ids, sc, ln = random_lists(rng, world, B, k, rows, tie_levels=11)
    base = np.arange(world, dtype=np.int32) * rows
    got = engine.shard_merge_topk(_dev(pack_rows(ids, sc, ln)), B, world, k, base)
    torch.cuda.synchronize()
    _same(_cpu(got), merge_batch(ids, sc, ln, base, k))
    for w, kk in ((14, 1024), (2, 1025), (65, 1)):
        rows_dev = torch.zeros((w, 1, engine.topk_row_bytes(kk)), dtype=torch.uint8, device="cuda")
        with pytest.raises(_lib.ErhError) as e:
            engine.shard_merge_topk(rows_dev, 1, w, kk, np.zeros(w, np.int32))
        assert e.value.status == _lib.ERH_ERR_UNSUPPORTED and "163840" in str(e.value) and "1024" in str(e.value)
    rs = torch.zeros((14, 1, engine.topk_row_bytes(1024)), dtype=torch.uint8, device="cuda")
    rd = torch.zeros((14, 1, engine.topk_row_bytes(288)), dtype=torch.uint8, device="cuda")
    with pytest.raises(_lib.ErhError) as e:
        engine.shard_rrf(rs, 1024, rd, 288, 1, 14, np.zeros(14, np.int32))
    assert e.value.status == _lib.ERH_ERR_UNSUPPORTED
    rd = torch.zeros((2, 1, engine.topk_row_bytes(769)), dtype=torch.uint8, device="cuda")
    rs = torch.zeros((2, 1, engine.topk_row_bytes(10)), dtype=torch.uint8, device="cuda")
    with pytest.raises(_lib.ErhError) as e:                                             # erh_hybrid_topk's own limit
        engine.shard_rrf(rs, 10, rd, 769, 1, 2, np.zeros(2, np.int32))
    assert e.value.status == _lib.ERH_ERR_UNSUPPORTED


def test_shard_rrf_ids_outside_the_content_table_end_their_list(engine):
    """A wrong id_base must not become a read outside content_id: the list ends in front of the first id outside the table."""
    import torch
    world, B, k = 2, 1, 4
    ids = np.array([[[0, 1, 2, 3]], [[0, 1, 2, 3]]], np.int32)
    sc = np.array([[[4.0, 3.0, 2.0, 1.0]], [[3.5, 2.5, 1.5, 0.5]]])
    ln = np.array([[4], [4]], np.int32)
    engine.set_shard_content(np.arange(6, dtype=np.int32))                              # documents 0 .. 5 only
    try:
        rows = _dev(pack_rows(ids, sc, ln))
        got = _cpu(engine.shard_rrf(rows, k, rows, k, B, world, np.array([0, 4], np.int32), K=60, topk=8))
        torch.cuda.synchronize()
    finally:
        engine.set_shard_content(None)
    assert got[2][0] == 4 and list(got[0][0, :4]) == [0, 4, 1, 5]                       # rank 1 contributes ids 4, 5 and stops


# ---- the layout against the unsharded engine -------------------------------------------------------------------------------------

N_W, D_W, VOCAB_W, B_W = 30000, 256, 3000, 1003                                         # the workload of tests/test_gpu_dist.py


@pytest.fixture(scope="module")
def workload():
    x = synth.dense_corpus(N_W, D_W, seed=11)
    q = synth.dense_queries(x, B_W, seed=12).astype(np.float16)
    flat, lens = synth.token_corpus(N_W, VOCAB_W, seed=13, mean_len=24)
    docs = [list(map(int, t)) for t in synth.split_docs(flat, lens)]
    idx = {v: build_bm25_index(docs, v) for v in (BM25S, OKAPI)}
    queries = [idx[BM25S].tokens_to_ids(list(map(int, t))) for t in synth.token_queries(flat, lens, VOCAB_W, B_W, seed=14)]
    rng = np.random.default_rng(15)
    cid = np.arange(N_W, dtype=np.int32)                                                # 1 % duplicated contents, anywhere in the corpus
    dup = rng.choice(N_W, size=N_W // 100, replace=False)
    cid[dup] = np.minimum(cid[dup], rng.integers(0, N_W, size=dup.shape[0]))
    return dict(x=x, q=q, idx=idx, queries=queries, cid=cid, csr=queries_to_csr(queries))


ROUTES = ("dense", "bm25_192", "bm25_1024", "hybrid_10", "hybrid_256")


def _calls(w, variant):
    """route name -> f(target) with target a RetrievalEngine (host outputs) or a CorpusShards (device tensors)."""
    qi, qt = w["csr"]
    return {
        "dense": lambda t: t.dense_topk(w["q"], 288),
        "bm25_192": lambda t: t.bm25_topk(qi, qt, 192),
        "bm25_1024": lambda t: t.bm25_topk(qi, qt, 1024),
        "hybrid_10": lambda t: t.hybrid_topk(w["q"], qi, qt, k_dense=288, k_sparse=192, K=60, topk=10),
        "hybrid_256": lambda t: t.hybrid_topk(w["q"], qi, qt, k_dense=288, k_sparse=192, K=60, topk=256),
    }


@pytest.fixture(scope="module")
def unsharded(engine, workload):
    """The parent path: the whole corpus in one handle, every route, both variants."""
    w, out = workload, {}
    engine.set_dense(w["x"])
    engine.set_doc_meta(N_W, w["cid"], None)
    for v in (BM25S, OKAPI):
        engine.set_bm25(w["idx"][v])
        for name, f in _calls(w, v).items():
            out[v, name] = tuple(np.array(a) for a in f(engine))
    return out


def _engines(world):
    made = []
    try:
        for _ in range(world):
            made.append(RetrievalEngine(0))
    except Exception:
        for e in made:
            e.close()
        raise
    return made


def _sparse_scores(idx, q_tokens):
    acc = np.zeros(idx.n_docs, np.float64 if idx.variant == OKAPI else np.float32)
    for t in q_tokens:
        s, e = idx.indptr[t], idx.indptr[t + 1]
        np.add.at(acc, idx.doc_ids[s:e], idx.payload[s:e])
    return acc


@pytest.mark.parametrize("world", [1, 3, 8])
@pytest.mark.parametrize("variant", [BM25S, OKAPI], ids=["bm25s", "okapi"])
def test_slices_on_one_device_equal_the_unsharded_engine(workload, unsharded, variant, world):
    import torch
    w = workload
    engines = _engines(world)
    try:
        cs = erd.CorpusShards.local(N_W, engines)
        cs.load(w["x"], w["idx"][variant], w["cid"], None)
        assert [e.n_dense for e in engines] == [hi - lo for lo, hi in (erd.corpus_shard_bounds(N_W, r, world) for r in range(world))]
        got = {}
        for name, f in _calls(w, variant).items():
            got[name] = _cpu(f(cs))                                                     # (.cpu() synchronises)
            if name != "bm25_192" and name != "bm25_1024":
                for e in engines:
                    assert e.dense_diag()["uncertified"] == 0
            _same(got[name], unsharded[variant, name], f"{name} world={world}")
        assert cs.transport == "device-copy"
        # ... and the oracle composition on the queries a sample draws
        idx = w["idx"][variant]
        for b in range(0, B_W, 143):
            sp = bm25_filter(_sparse_scores(idx, w["queries"][b]), 192)
            did, dsc = dense_exact_topk(w["x"], w["q"][b], 288)
            assert list(got["dense"][0][b]) == list(did) and list(got["dense"][1][b]) == list(dsc)
            assert list(got["bm25_192"][0][b, :len(sp)]) == [i for i, _ in sp] and got["bm25_192"][2][b] == len(sp)
            want = reciprocal_rank_fusion([[Item(i, int(w["cid"][i]), s) for i, s in sp],
                                           [Item(int(i), int(w["cid"][i]), float(s)) for i, s in zip(did, dsc)]], K=60, topk=256)
            assert list(got["hybrid_256"][0][b, :len(want)]) == [x.idx for x in want]
            assert list(got["hybrid_256"][1][b, :len(want)]) == [x.score for x in want]
        if variant == BM25S:
            # dense FAST: scores within 1e-3 of the exact ones and sorted (tests/test_gpu_dense.py's rule; see the module docstring)
            fid, fsc, fln = _cpu(cs.dense_topk(w["q"][:64], 100, mode=_lib.ERH_DENSE_FAST))
            assert np.all(fln == 100)
            for i in range(0, 64, 9):
                exact = dense_exact_scores(w["x"], w["q"][i], rows=fid[i])
                assert np.max(np.abs(fsc[i] - exact)) < 1e-3 and np.all(np.diff(fsc[i]) <= 0)
                assert len(set(fid[i]) & set(unsharded[variant, "dense"][0][i, :100])) >= 98
    finally:
        for e in engines:
            e.close()


def test_raw_abi_path_and_second_call_equal_the_layout(workload, unsharded):
    """Three handles on device 0 driven by hand through the C ABI -- per slice: route calls with device outputs, dense_check,
    erh_pack_topk into the rank's block; then erh_shard_rrf -- and CorpusShards.local called twice (the second call reuses its
    buffers) give the unsharded hybrid result."""
    import torch
    from easyrag_amd.index import slice_bm25_index
    w, world = workload, 3
    qi, qt = w["csr"]
    qd = _dev(w["q"])
    engines = _engines(world)
    try:
        base = np.array([erd.corpus_shard_bounds(N_W, r, world)[0] for r in range(world)], np.int32)
        rs = torch.empty((world, B_W, engines[0].topk_row_bytes(192)), dtype=torch.uint8, device="cuda")
        rd = torch.empty((world, B_W, engines[0].topk_row_bytes(288)), dtype=torch.uint8, device="cuda")
        for r, e in enumerate(engines):
            lo, hi = erd.corpus_shard_bounds(N_W, r, world)
            e.set_dense(w["x"][lo:hi])
            e.set_bm25(slice_bm25_index(w["idx"][BM25S], lo, hi), payload_on_device=True)   # global idf / avgdl on the device
            s = e.bm25_topk(qi, qt, 192, device_out=True)
            d = e.dense_topk(qd, 288, device_out=True)
            e.dense_check()
            e.pack_topk(*s, rs[r])
            e.pack_topk(*d, rd[r])
        engines[1].set_shard_content(w["cid"])                                          # any handle may merge
        got = _cpu(engines[1].shard_rrf(rs, 192, rd, 288, B_W, world, base, K=60, topk=10))
        _same(got, unsharded[BM25S, "hybrid_10"], "raw ABI")
        cs = erd.CorpusShards.local(N_W, engines)
        cs.load(content_id=w["cid"])
        for _ in range(2):
            got = _cpu(cs.hybrid_topk(qd, qi, qt, k_dense=288, k_sparse=192, K=60, topk=10))
            _same(got, unsharded[BM25S, "hybrid_10"], "CorpusShards.local")
    finally:
        for e in engines:
            e.close()


def test_edge_shapes(engine):
    """1000 rows over 8 slices of 125: lists shorter than k on every slice; duplicated rows in different slices (tie order by global id);
    per-query dir filters with one class inside a single slice and one spread over all; BM25 lists empty on every slice."""
    n, d, vocab, B, world = 1000, 256, 300, 48, 8
    rng = np.random.default_rng(8)
    x = synth.dense_corpus(n, d, seed=31)
    x[910] = x[10]
    x[500] = x[10]                                                                      # one row three times: slices 0, 4, 7
    x[377] = x[376]
    q = synth.dense_queries(x, B, seed=32).astype(np.float16)
    q[0] = x[10]
    q[1] = x[376]
    flat, lens = synth.token_corpus(n, vocab, seed=33, mean_len=12)
    docs = [list(map(int, t)) for t in synth.split_docs(flat, lens)]
    docs[910], docs[500] = list(docs[10]), list(docs[10])                               # ... and equal BM25 scores across slices
    idx = build_bm25_index_from_ids(docs, vocab + 5, BM25S)                            # 5 terms no document holds
    queries = [list(map(int, t)) for t in synth.token_queries(flat, lens, vocab, B, seed=34)]
    queries[0] = list(docs[10][:6])
    queries[2] = []                                                                     # no tokens: empty on every slice
    queries[3] = [vocab + 1, vocab + 4]                                                 # tokens no document holds: likewise
    qi, qt = queries_to_csr(queries)
    dir_id = np.full(n, 2, np.int16)
    dir_id[260:300] = 0                                                                 # class 0: inside slice 2 (rows 250 .. 374)
    dir_id[rng.choice(n, size=200, replace=False)] = 1                                  # class 1: everywhere
    dir_id[260:300] = 0
    filt = (np.arange(B) % 4 - 1).astype(np.int16)                                      # -1 (none), 0, 1, 2
    filt_dense = np.roll(filt, 1)
    cid = np.arange(n, dtype=np.int32)
    cid[910] = 10                                                                       # one content in slices 0 and 7
    engine.set_dense(x)
    engine.set_bm25(idx)
    engine.set_doc_meta(n, cid, dir_id)
    want = {
        "dense": engine.dense_topk(q, 288),
        "dense_f": engine.dense_topk(q, 288, filter_dir=filt),
        "bm25": engine.bm25_topk(qi, qt, 192),
        "bm25_f": engine.bm25_topk(qi, qt, 192, filter_dir=filt),
        "hybrid": engine.hybrid_topk(q, qi, qt, k_dense=288, k_sparse=192, K=60, topk=256),
        "hybrid_f": engine.hybrid_topk(q, qi, qt, k_dense=288, k_sparse=192, K=60, topk=10, filter_dir=filt, filter_dense=filt_dense),
    }
    want = {k: tuple(np.array(a) for a in v) for k, v in want.items()}
    assert np.all(want["dense"][2] == 288) and want["bm25"][2][2] == 0 and want["bm25"][2][3] == 0
    assert list(want["dense"][0][0, :3]) == [10, 500, 910] and list(want["dense"][0][1, :2]) == [376, 377]
    engines = _engines(world)
    try:
        cs = erd.CorpusShards.local(n, engines)
        cs.load(x, idx, cid, dir_id)
        got = {
            "dense": cs.dense_topk(q, 288),
            "dense_f": cs.dense_topk(q, 288, filter_dir=filt),
            "bm25": cs.bm25_topk(qi, qt, 192),
            "bm25_f": cs.bm25_topk(qi, qt, 192, filter_dir=filt),
            "hybrid": cs.hybrid_topk(q, qi, qt, k_dense=288, k_sparse=192, K=60, topk=256),
            "hybrid_f": cs.hybrid_topk(q, qi, qt, k_dense=288, k_sparse=192, K=60, topk=10, filter_dir=filt, filter_dense=filt_dense),
        }
        for name in want:
            _same(_cpu(got[name]), want[name], name)
        # every slice answered with its 125 rows; class 0 has rows in slice 2 only
        ids, sc, ln = engines[5].dense_topk(q, 288)
        assert np.all(ln == 125)
        ids, sc, ln = engines[5].dense_topk(q[:4], 288, filter_dir=np.zeros(4, np.int16))
        assert np.all(ln == 0)
    finally:
        for e in engines:
            e.close()
    with pytest.raises(ValueError):
        erd.CorpusShards.local(2, [None, None, None])                                   # an empty slice


def test_two_processes_on_the_one_gpu():
    """Two ranks under torch.distributed.run on device 0 (gloo: RCCL does not share a device between ranks; the packed rows cross through
    pinned host memory): every rank holds half the corpus and must end with the unsharded result (tests/_corpus_shard_rank_main.py)."""
    import os
    import socket
    import subprocess
    import sys
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_corpus_shard_rank_main.py")
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr",
                        "127.0.0.1", "--master-port", str(port), script], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "CORPUS-SHARDS-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    assert "gloo-staged" in r.stdout


# ---- full size ---------------------------------------------------------------------------------------------------------------------

def test_full_size_four_slices(engine):
    """BASELINE.json's full size -- 1 M x 1024 chunks, the ~60 M-posting index -- in 4 slices on the one device: hybrid at B = 256 and
    dense at B = 1 equal the unsharded calls bit for bit, and no query of any slice went to the exhaustive path (the slices are
    contiguous quarters of an i.i.d. corpus: what tests/test_gpu_fullsize.py asserts of the whole corpus must hold of them)."""
    import torch
    N, D, VOCAB, world = 1_000_000, 1024, 262_144, 4
    dev = torch.device("cuda", 0)
    x = synth.dense_corpus_torch(N, D, seed=2, device=dev)
    q = synth.dense_queries_torch(x, 256, seed=1000)
    indptr, doc, tf, lens, flat = synth.token_csr_torch(N, VOCAB, seed=3, device=dev)
    queries = synth.token_queries(flat, lens, VOCAB, 256, seed=2000)
    del flat
    torch.cuda.empty_cache()
    idx = build_bm25_index_from_postings(indptr, doc, tf, lens, BM25S, compute_payload=False)
    qi, qt = queries_to_csr(queries)
    engine.set_dense(x)
    engine.set_bm25(idx, payload_on_device=True)
    engine.set_doc_meta(N, None, None)
    engine.reset_stats()
    want_h = engine.hybrid_topk(q, qi, qt, k_dense=288, k_sparse=192, K=60, topk=10)
    want_d = engine.dense_topk(q[:1].contiguous(), 288)
    assert engine.stat("dense_exhaustive_queries") == 0
    engines = _engines(world)
    try:
        cs = erd.CorpusShards.local(N, engines)
        cs.load(x, idx, None, None, payload_on_device=True)
        for e in engines:
            e.reset_stats()
        got_h = _cpu(cs.hybrid_topk(q, qi, qt, k_dense=288, k_sparse=192, K=60, topk=10))
        diag_h = [e.dense_diag() for e in engines]
        got_d = _cpu(cs.dense_topk(q[:1].contiguous(), 288))
        diag_d = [e.dense_diag() for e in engines]
        stats = [e.stats() for e in engines]
        print("full-size slices: exhaustive queries per slice", [s["dense_exhaustive_queries"] for s in stats], diag_h, diag_d)
        _same(got_h, tuple(np.array(a) for a in want_h), "hybrid B=256")
        _same(got_d, tuple(np.array(a) for a in want_d), "dense B=1")
        for s, dh, dd in zip(stats, diag_h, diag_d):
            assert dh["uncertified"] == 0 and dd["uncertified"] == 0
            assert s["dense_exhaustive_queries"] == 0 and dh["exhaustive"] == 0 and dd["exhaustive"] == 0, (s, dh, dd)
    finally:
        for e in engines:
            e.close()
