"""One rank of tests/test_gpu_corpus_shards.py::test_two_processes_on_the_one_gpu (run under torch.distributed.run, both ranks on
device 0, gloo): the corpus cut in two, every rank holding its half in its own handle, CorpusShards gathering the packed lists
through pinned host memory; every rank must end with the result of the unsharded call, which each computes in a handle of its own."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from easyrag_amd import dist as erd, synth                      # noqa: E402
from easyrag_amd.engine import RetrievalEngine, queries_to_csr    # noqa: E402
from easyrag_amd.index import BM25S, build_bm25_index             # noqa: E402


def main():
    rank, world = erd.init_from_env(device_index=0, backend="gloo")
    torch.cuda.set_device(0)
    n, d, vocab, B = 20001, 256, 2000, 301                          # ragged halves
    x = synth.dense_corpus(n, d, seed=21)
    q = torch.from_numpy(synth.dense_queries(x, B, seed=22).astype(np.float16)).cuda()
    flat, lens = synth.token_corpus(n, vocab, seed=23, mean_len=24)
    idx = build_bm25_index([list(map(int, t)) for t in synth.split_docs(flat, lens)], BM25S)
    queries = [idx.tokens_to_ids(list(map(int, t))) for t in synth.token_queries(flat, lens, vocab, B, seed=24)]
    qi, qt = queries_to_csr(queries)
    cid = np.arange(n, dtype=np.int32)
    cid[n - 5] = 3                                                  # one content in both halves
    dir_id = (np.arange(n) % 3).astype(np.int16)
    filt = (np.arange(B) % 4 - 1).astype(np.int16)

    full = RetrievalEngine(0)
    full.set_dense(x)
    full.set_bm25(idx)
    full.set_doc_meta(n, cid, dir_id)
    want = {"hybrid": full.hybrid_topk(q, qi, qt, k_dense=288, k_sparse=192, K=60, topk=10),
            "hybrid_f": full.hybrid_topk(q, qi, qt, k_dense=288, k_sparse=192, K=60, topk=256, filter_dir=filt),
            "dense": full.dense_topk(q, 288), "bm25": full.bm25_topk(qi, qt, 1024)}
    full.close()

    eng = RetrievalEngine(0)
    info = {}
    for mode in ("torch", "native"):
        cs = erd.CorpusShards(n, rank, world, engine=eng, mode=mode)
        cs.load(x, idx, cid, dir_id)
        assert eng.n_dense == cs.bounds[1] - cs.bounds[0]
        for _ in range(2):                                          # the second round reuses the buffers
            got = {"hybrid": cs.hybrid_topk(q, qi, qt, k_dense=288, k_sparse=192, K=60, topk=10),
                   "hybrid_f": cs.hybrid_topk(q, qi, qt, k_dense=288, k_sparse=192, K=60, topk=256, filter_dir=filt),
                   "dense": cs.dense_topk(q, 288), "bm25": cs.bm25_topk(qi, qt, 1024)}
        torch.cuda.synchronize()
        for name, w in want.items():
            g = got[name]
            ok = (np.array_equal(g[0].cpu().numpy(), w[0]) and np.array_equal(g[2].cpu().numpy(), w[2]) and
                  np.array_equal(g[1].cpu().numpy().view(np.uint64), w[1].view(np.uint64)))
            if not ok:
                raise SystemExit(f"rank {rank}: {name} (mode {mode}, ran as {cs.mode}) differs from the unsharded result")
        info[mode] = (cs.mode, cs.transport, cs.fallback_reason is not None)
    if world > 1:
        torch.distributed.barrier()
    if rank == 0:
        print("CORPUS-SHARDS-OK " + repr(info), flush=True)
    if world > 1:
        torch.distributed.destroy_process_group()
    eng.close()


if __name__ == "__main__":
    main()
