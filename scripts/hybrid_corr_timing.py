#!/usr/bin/env python
"""What hybrid_lazy is worth when the two routes AGREE: the headline step (1024 queries, dense top-288 + BM25 top-192 -> RRF(60) -> top-10,
1M x 1024 chunks) with correlated routes, beside the benchmark's independent ones.

The benchmark draws the dense target and the token target of a query independently, so the join of the two route lists is nearly empty
and the lazy final kernel re-scores the prefix window only.  Here every query's token targets and dense near-copies are the SAME documents:
the sparse route's own list is computed first, and `--targets` of its documents (every third rank) are overwritten with unit rows at cosines
spread over [--cos-lo, --cos-hi] to the query (orthogonal noise: the cosine is what is asked for), which puts them at dense ranks from
about 250 up to the top.  The lazy kernel then owes an exact rank to every joined row and re-scores its 2 delta window.

Arms hybrid_lazy = 0 / 1, interleaved (a b | b a | ...; visit 0 is a warm-up), --reps visits of --steps calls each; per arm the median /
min / max ms per step (wall clock around device-output calls, one synchronisation per visit), the final kernels' re-scored rows per query
(erh_get_stat dense_rescored_rows_last_call) and the size of the join; the arms' results are compared bit for bit.

  python scripts/hybrid_corr_timing.py [--out profiles/hybrid_corr_timing.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--vocab", type=int, default=262_144)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--targets", type=int, default=60)
    ap.add_argument("--cos-lo", type=float, default=0.100)
    ap.add_argument("--cos-hi", type=float, default=0.160)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from easyrag_amd import synth
    from easyrag_amd.engine import RetrievalEngine, queries_to_csr
    from easyrag_amd.index import BM25S, build_bm25_index_from_postings
    dev = torch.device("cuda", 0)
    n, d, B, kd, ks = args.chunks, args.dim, args.batch, 288, 192
    eng = RetrievalEngine(0)
    x = synth.dense_corpus_torch(n, d, seed=2, device=dev)
    q = synth.dense_queries_torch(x, B, seed=1000)
    indptr, doc, tf, lens, flat = synth.token_csr_torch(n, args.vocab, seed=3, device=dev)
    eng.set_bm25(build_bm25_index_from_postings(indptr, doc, tf, lens, BM25S, compute_payload=False), payload_on_device=True)
    csr = queries_to_csr(synth.token_queries(flat, lens, args.vocab, B, seed=2000))
    eng.set_doc_meta(n, None, None)
    sync = torch.cuda.synchronize

    def measure(label):
        ms, rows, outs = {0: [], 1: []}, {}, {}
        for rep in range(args.reps + 1):
            for lazy in ((0, 1) if rep % 2 == 0 else (1, 0)):
                eng.set_option("hybrid_lazy", lazy)
                out = eng.hybrid_topk(q, *csr, k_dense=kd, k_sparse=ks, K=60, topk=10, device_out=True)
                sync()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    out = eng.hybrid_topk(q, *csr, k_dense=kd, k_sparse=ks, K=60, topk=10, device_out=True)
                sync()
                dt = (time.perf_counter() - t0) / args.steps * 1e3
                eng.dense_check()
                if rep == 0:
                    rows[lazy] = eng.stat("dense_rescored_rows_last_call") / B
                    outs[lazy] = [t.cpu().numpy().copy() for t in out]
                else:
                    ms[lazy].append(dt)
        same = all(a.tobytes() == b.tobytes() for a, b in zip(outs[0], outs[1]))
        rec = {"results_identical": same}
        for lazy in (0, 1):
            rec[f"hybrid_lazy={lazy}"] = {"median_ms": statistics.median(ms[lazy]), "min_ms": min(ms[lazy]), "max_ms": max(ms[lazy]),
                                          "visits": len(ms[lazy]), "rescored_rows_per_query": rows[lazy]}
        rec["delta_of_medians_pct"] = round(100.0 * (rec["hybrid_lazy=1"]["median_ms"] / rec["hybrid_lazy=0"]["median_ms"] - 1.0), 2)
        print(label, json.dumps(rec), flush=True)
        return rec

    def join_size():
        s_ids, _, s_len = eng.bm25_topk(*csr, ks)
        d_ids, _, d_len = eng.dense_topk(q, kd)
        return float(np.mean([len(set(s_ids[b, :s_len[b]]) & set(d_ids[b, :d_len[b]])) for b in range(B)])), s_ids, s_len

    report = {"shape": {"chunks": n, "dim": d, "batch": B, "k_dense": kd, "k_sparse": ks, "K": 60, "topk": 10, "steps": args.steps, "reps": args.reps}}
    eng.set_dense(x)
    join, s_ids, s_len = join_size()
    report["independent"] = {"joined_documents_per_query": join, **measure("independent")}
    # correlate: the query's sparse ranks 1, 4, 7, ... become its dense near-copies, cosine rising towards the best sparse ranks
    T = args.targets
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    cos = torch.linspace(args.cos_hi, args.cos_lo, T, device=dev)[None, :, None]
    qf = q.float()
    for b0 in range(0, B, 128):                                        # (B x T x d floats at once is 250 MB: in slices)
        b1 = min(B, b0 + 128)
        r = torch.randn((b1 - b0, T, d), generator=g, device=dev)
        qq = qf[b0:b1, None, :]
        u = r - (r * qq).sum(-1, keepdim=True) * qq
        u = u / u.norm(dim=-1, keepdim=True)
        rows = (cos * qq + torch.sqrt(1.0 - cos * cos) * u).to(torch.float16)
        for b in range(b0, b1):
            m = min(T, int(s_len[b]) // 3)
            if m > 0:
                x[torch.from_numpy(s_ids[b, 0:3 * m:3].astype(np.int64)).to(dev)] = rows[b - b0, :m]
    eng.set_dense(x)
    join, _, _ = join_size()
    report["correlated"] = {"joined_documents_per_query": join, "targets": T, "cos": [args.cos_lo, args.cos_hi], **measure("correlated")}
    report["stats"] = {k: v for k, v in eng.stats().items() if k in ("hybrid_calls", "hybrid_lazy_queries", "dense_exhaustive_queries")}
    eng.close()
    text = json.dumps(report, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
