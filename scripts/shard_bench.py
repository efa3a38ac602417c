#!/usr/bin/env python
"""What the corpus-sharded layout (dist.CorpusShards) costs and buys, measured on ONE card: the configs[3] corpus (1M x 1024 chunks, the
~60 M-posting bm25s index), B = 1 and B = 1024, routes `hybrid` (BM25 192 + dense 288 -> RRF top 10) and `dense` (k = 288).

  (a) the unsharded step in this process with this timing code -- the yardstick;
  (b) for world in {2, 4, 8}: every slice's own step (its handle holds N / world rows; route calls with device outputs, erh_dense_check,
      erh_pack_topk), the slices run one after the other;
  (c) the merge / fuse kernels on the gathered rows (erh_shard_rrf, erh_shard_merge_topk) by HIP events, beside erh_rrf on the same batch.

Arms are visited interleaved (a b c | c b a | ...; visit 0 warms up and sizes the visits), every arm gets >= --min-seconds of timed work,
the report is median / min / max ms per step over the visits.  `projection_ms` = max over slices + merge: a PROJECTION of the multi-GPU
step -- no run on more than one GPU is behind it and the exchange is not in it.

  python scripts/shard_bench.py [--worlds 2,4,8] [--batches 1,1024] [--out profiles/<name>.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from easyrag_amd import dist as erd, synth  # noqa: E402
from easyrag_amd.engine import RetrievalEngine, queries_to_csr  # noqa: E402
from easyrag_amd.index import BM25S, build_bm25_index_from_postings  # noqa: E402

K_DENSE, K_SPARSE, TOPK = 288, 192, 10


def summary(v, steps):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "visits": len(v), "steps_per_visit": steps}


def timed_arms(arms, reps, base_steps, min_seconds):
    """arms: {name: step()} -> {name: summary}; wall clock around `steps` calls, device idle before and after."""
    names = list(arms)
    ms = {a: [] for a in names}
    steps = {a: base_steps for a in names}
    for rep in range(reps + 1):
        for a in (names if rep % 2 == 0 else names[::-1]):
            arms[a]()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps[a]):
                arms[a]()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if rep == 0:
                steps[a] = max(base_steps, int(np.ceil(min_seconds / reps / (dt / steps[a]))))
                continue
            ms[a].append(dt / steps[a] * 1e3)
    return {a: summary(ms[a], steps[a]) for a in names}


def event_ms(fn, reps, inner):
    """Kernel-side time of fn() by HIP events: `inner` back-to-back calls between two events, `reps` times."""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / inner)
    return summary(out, inner)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--vocab", type=int, default=262_144)
    ap.add_argument("--worlds", default="2,4,8")
    ap.add_argument("--batches", default="1,1024")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    worlds = [int(w) for w in args.worlds.split(",") if w]
    batches = [int(b) for b in args.batches.split(",") if b]
    dev = torch.device("cuda", 0)
    n, d = args.chunks, args.dim
    x = synth.dense_corpus_torch(n, d, seed=2, device=dev)
    q_all = synth.dense_queries_torch(x, max(batches), seed=1000)
    indptr, doc, tf, lens, flat = synth.token_csr_torch(n, args.vocab, seed=3, device=dev)
    idx = build_bm25_index_from_postings(indptr, doc, tf, lens, BM25S, compute_payload=False)
    tok_all = synth.token_queries(flat, lens, args.vocab, max(batches), seed=2000)
    del flat
    torch.cuda.empty_cache()

    def route_step(eng, route, q, qi, qt, pack=None):
        """One engine's step on what it holds: the route's device lists, certified; packed when the rows are to travel."""
        lists = []
        if route == "hybrid" and pack is None:
            out = eng.hybrid_topk(q, qi, qt, k_dense=K_DENSE, k_sparse=K_SPARSE, K=60, topk=TOPK, device_out=True)
            eng.dense_check()
            return out
        if route == "hybrid":
            lists.append(eng.bm25_topk(qi, qt, K_SPARSE, device_out=True))
        lists.append(eng.dense_topk(q, K_DENSE, device_out=True))
        eng.dense_check()
        if pack is not None:
            for (ids, sc, ln), rows in zip(lists, pack):
                eng.pack_topk(ids, sc, ln, rows)
        return lists[-1]

    full = RetrievalEngine(0)
    full.set_dense(x)
    full.set_bm25(idx, payload_on_device=True)
    full.set_doc_meta(n, None, None)
    rec = {"shape": {"chunks": n, "dim": d, "vocab": args.vocab, "postings": int(idx.nnz), "k_dense": K_DENSE, "k_sparse": K_SPARSE,
                     "topk": TOPK, "variant": "bm25s"},
           "note": "slices run one after the other on one card; projection_ms = max(slice) + merge, exchange not included, not a multi-GPU run",
           "runs": []}
    for world in [1] + worlds:
        engines = [full] if world == 1 else [RetrievalEngine(0) for _ in range(world)]
        try:
            cs = None
            if world > 1:
                cs = erd.CorpusShards.local(n, engines)
                cs.load(x, idx, None, None, payload_on_device=True)
            for B in batches:
                q = q_all[:B].contiguous()
                qi, qt = queries_to_csr(tok_all[:B])
                for route in ("hybrid", "dense"):
                    if world == 1:
                        r = timed_arms({"unsharded": lambda: route_step(full, route, q, qi, qt)}, args.reps, args.steps, args.min_seconds)
                        entry = {"world": 1, "batch": B, "route": route, "unsharded": r["unsharded"]}
                        if route == "hybrid":                                      # erh_rrf on the same batch, for (c)
                            s = full.bm25_topk(qi, qt, K_SPARSE, device_out=True)
                            dn = full.dense_topk(q, K_DENSE, device_out=True)
                            full.dense_check()
                            entry["erh_rrf_event"] = event_ms(lambda: full.rrf_device(s[0], s[2], dn[0], dn[2], K=60, topk=TOPK), args.reps, 20)
                        rec["runs"].append(entry)
                        continue
                    ks = [K_SPARSE, K_DENSE] if route == "hybrid" else [K_DENSE]
                    rows = [torch.empty((world, B, full.topk_row_bytes(k)), dtype=torch.uint8, device=dev) for k in ks]
                    arms = {f"slice{r}": (lambda r=r: route_step(engines[r], route, q, qi, qt, pack=[t[r] for t in rows])) for r in range(world)}
                    per = timed_arms(arms, args.reps, args.steps, args.min_seconds)
                    if route == "hybrid":
                        merge = event_ms(lambda: engines[0].shard_rrf(rows[0], K_SPARSE, rows[1], K_DENSE, B, world, cs.id_base, K=60, topk=TOPK),
                                         args.reps, 20)
                    else:
                        merge = event_ms(lambda: engines[0].shard_merge_topk(rows[0], B, world, K_DENSE, cs.id_base), args.reps, 20)
                    whole = timed_arms({"all": lambda: (cs.hybrid_topk(q, qi, qt, k_dense=K_DENSE, k_sparse=K_SPARSE, K=60, topk=TOPK)
                                                       if route == "hybrid" else cs.dense_topk(q, K_DENSE))},
                                       args.reps, max(args.steps // 2, 2), args.min_seconds)
                    slowest = max(v["median_ms"] for v in per.values())
                    rec["runs"].append({"world": world, "batch": B, "route": route, "slices": per, "max_slice_median_ms": slowest,
                                        "merge_event": merge, "projection_ms": slowest + merge["median_ms"],
                                        "sequential_whole_call": whole["all"],
                                        "exchange_bytes": int(world * B * sum(ks) * 12),
                                        "stats_slice0": engines[0].stats()})
        finally:
            if world > 1:
                for e in engines:
                    e.close()
    full.close()
    txt = json.dumps(rec, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
