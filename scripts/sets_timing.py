#!/usr/bin/env python
"""Cost of the dense route's set filters (erh_dense_topk_sets) at the headline corpus shape: 1M x 1024 chunks in four contiguous dir
blocks (the reference's loader walks one directory after the other), 1024 queries, dense route alone and the hybrid (BM25 192 + dense
288 -> RRF top 10).  Arms, interleaved (a b c d | d c b a | ...; visit 0 is a warm-up): (i) unfiltered, (ii) one dir per query (today's
class column), (iii) MatchAny of 2 of the 4 dirs, (iv) must_not of 1 of the 4 dirs.  Every step ends with erh_dense_check (what a caller
of device outputs must do); each arm gets >= `--min-seconds` of timed work; the report is the median / min / max ms per step.

  python scripts/sets_timing.py [--arms dense_iii,hybrid_iii] [--out profiles/<name>.json]
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

from easyrag_amd import synth  # noqa: E402
from easyrag_amd.engine import RetrievalEngine, queries_to_csr  # noqa: E402
from easyrag_amd.index import BM25S, build_bm25_index_from_postings  # noqa: E402

ARMS = ("dense_i", "dense_ii", "dense_iii", "dense_iv", "hybrid_i", "hybrid_ii", "hybrid_iii", "hybrid_iv")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--vocab", type=int, default=262_144)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--dirs", type=int, default=4)
    ap.add_argument("--arms", default=",".join(ARMS))
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--min-seconds", type=float, default=0.3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    arms = [a for a in args.arms.split(",") if a]
    dev = torch.device("cuda", 0)
    n, d, B, D = args.chunks, args.dim, args.batch, args.dirs
    eng = RetrievalEngine(0)
    x = synth.dense_corpus_torch(n, d, seed=2, device=dev)
    eng.set_dense(x)
    q = synth.dense_queries_torch(x, B, seed=1000)
    hybrid = any(a.startswith("hybrid") for a in arms)
    if hybrid:
        indptr, doc, tf, lens, flat = synth.token_csr_torch(n, args.vocab, seed=3, device=dev)
        eng.set_bm25(build_bm25_index_from_postings(indptr, doc, tf, lens, BM25S, compute_payload=False), payload_on_device=True)
        qi, qt = queries_to_csr(synth.token_queries(flat, lens, args.vocab, B, seed=2000))
    eng.set_doc_meta(n, None, (np.arange(n) * D // n).astype(np.int16))
    one = (np.arange(B) % D).astype(np.int16)
    any2 = [[b % D, (b + 1) % D] for b in range(B)]
    not1 = [[c for c in range(D) if c != b % D] for b in range(B)]
    dense_sets = {"dense_iii": any2, "dense_iv": not1}
    col = {"i": None, "ii": one}

    def step(arm):
        route, which = arm.split("_")
        if route == "dense":
            if which in col:
                out = eng.dense_topk(q, 288, filter_dir=col[which], device_out=True)
            else:
                out = eng.dense_topk_sets(q, 288, dense_sets[arm], device_out=True)
            eng.dense_check()
            return out
        if which in col:
            out = eng.hybrid_topk(q, qi, qt, k_dense=288, k_sparse=192, K=60, topk=10, filter_dir=None, filter_dense=col[which],
                                  device_out=True)
            eng.dense_check()
            return out
        sids, _, sln = eng.bm25_topk(qi, qt, 192, device_out=True)
        dids, _, dln = eng.dense_topk_sets(q, 288, any2 if which == "iii" else not1, device_out=True)
        eng.dense_check()
        out = eng.rrf_device(sids, sln, dids, dln, K=60, topk=10)
        eng.sync()
        return out

    ms = {a: [] for a in arms}
    steps = {a: args.steps for a in arms}
    for rep in range(args.reps + 1):
        for arm in (arms if rep % 2 == 0 else arms[::-1]):
            step(arm)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps[arm]):
                step(arm)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if rep == 0:                                   # warm-up visit: size the arm's visits so that it gets >= min-seconds of timed work
                steps[arm] = max(args.steps, int(np.ceil(args.min_seconds / args.reps / (dt / steps[arm]))))
                continue
            ms[arm].append(dt / steps[arm] * 1e3)
    rec = {"shape": {"chunks": n, "dim": d, "batch": B, "dirs": D, "layout": "contiguous blocks", "k_dense": 288, "k_sparse": 192, "topk": 10},
           "arms": {a: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "visits": len(v), "steps_per_visit": steps[a],
                        "timed_s": sum(v) * steps[a] / 1e3} for a, v in ms.items()},
           "stats": eng.stats()}
    txt = json.dumps(rec, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")
    eng.close()


if __name__ == "__main__":
    main()
