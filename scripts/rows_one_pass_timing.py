#!/usr/bin/env python
"""The rows entries as one pass per call (DESIGN K11, "One pass per call") against the parent commit's two-pass entries: same kernels, so
the difference is host work, copies and synchronisations.  1M rows; dense d = 1024, k = 100; BM25 (bm25s) over a 262144-term vocabulary, the
reference's question lengths, k = 192 -- the shapes of scripts/rows_scan_timing.py.  Four points per route:
  short      1024 queries, each on its own 256-row list (one more copy enqueued, one staging copy less)
  long_off   one 524288-row list shared by 16 queries, *_rows_scan = 0
  long_scan  the same list, *_rows_scan = 2
  hand_back  4 overlapping 131072-row lists, 16 queries, *_rows_scan = 1: the rule says yes before the cells are known and no after
Both trees run the same script: every visit is a child process that imports the library of ONE tree (--tree), builds the corpus, and times
the four points interleaved with the `timed` helper of scripts/rows_timing.py; the visits of the two trees alternate.  Per point and tree:
the median over the visits' medians and the visit-to-visit spread (max - min).  `within_bar`: this tree's median <= the parent's median + the
parent's own spread.  No threshold is enforced here: the record says what was found.

  python scripts/rows_one_pass_timing.py --parent DIR [--visits 3] [--out profiles/rows_one_pass_timing.json]
DIR: a checkout of the parent commit with its library built.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SECTIONS = ("dense", "bm25s")
POINTS = ("short", "long_off", "long_scan", "hand_back")
LIMIT_S = 240


def section(args):
    sys.path.insert(0, os.path.abspath(args.tree))
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import torch
    from rows_timing import timed
    from easyrag_amd import synth
    from easyrag_amd.engine import RetrievalEngine, queries_to_csr
    from easyrag_amd.index import BM25S, build_bm25_index_from_postings
    dev = torch.device("cuda", 0)
    n = args.rows
    dense = args.section == "dense"
    route = "dense" if dense else "bm25"
    eng = RetrievalEngine(0)
    if dense:
        x = synth.dense_corpus_torch(n, args.dim, seed=2, device=dev)
        eng.set_dense(x)
        qall = synth.dense_queries_torch(x, 1024, seed=1000)

        def call(B, csr):
            return eng.dense_topk_rows_csr(qall[:B], 100, *csr, device_out=True)
    else:
        indptr, doc, tf, lens, flat = synth.token_csr_torch(n, args.vocab, seed=3, device=dev)
        eng.set_bm25(build_bm25_index_from_postings(indptr, doc, tf, lens, BM25S, compute_payload=False), payload_on_device=True)
        queries = synth.token_queries(flat, lens, args.vocab, 1024, seed=2000, lengths=synth.REF_QUESTION_LENGTHS)
        qcsr = {B: queries_to_csr(queries[:B]) for B in (16, 1024)}
        del indptr, doc, tf, flat

        def call(B, csr):
            return eng.bm25_topk_rows_csr(*qcsr[B], 192, *csr, device_out=True)

    rng = np.random.default_rng(5)

    def pick(length):
        return np.sort(rng.choice(n, size=length, replace=False)).astype(np.int64)
    one = RetrievalEngine.lists_to_csr([pick(524288)], np.zeros(16, np.int32), 16)
    plan = {"short": (1024, RetrievalEngine.lists_to_csr([pick(256) for _ in range(1024)], None, 1024), 1),
            "long_off": (16, one, 0), "long_scan": (16, one, 2),
            "hand_back": (16, RetrievalEngine.lists_to_csr([pick(131072) for _ in range(4)], (np.arange(16) % 4).astype(np.int32), 16), 1)}

    def step(point):
        B, csr, scan = plan[point]
        eng.set_option(route + "_rows_scan", scan)
        out = call(B, csr)
        eng.sync()
        return out
    rec = timed(list(POINTS), step, torch.cuda.synchronize, 1, args.reps, args.min_seconds)
    for point in POINTS:                                                     # which shapes answered: the points are what they are named after
        before = {s: eng.stat(route + s) for s in ("_rows_scan_calls", "_rows_short_launches", "_rows_long_launches")}
        step(point)
        rec[point]["moved"] = {s: eng.stat(route + s) - v for s, v in before.items()}
    eng.close()
    with open(args.part, "w") as f:
        json.dump(rec, f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="checkout of the parent commit, library built")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--vocab", type=int, default=262_144)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--visits", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--min-seconds", type=float, default=0.1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rows_one_pass_timing.json"))
    ap.add_argument("--section", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--part", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.section:
        return section(args)
    if not args.parent:
        ap.error("--parent is required")
    trees = {"parent": os.path.abspath(args.parent), "this": ROOT}
    rec = {"shape": {"rows": args.rows, "dense": {"dim": args.dim, "k": 100}, "bm25": {"vocab": args.vocab, "k": 192, "variant": "bm25s",
                                                                                        "query_lengths": "the reference's 103 questions"}},
           "method": {"visits": args.visits, "reps": args.reps, "min_seconds": args.min_seconds,
                      "every step": "device outputs + one stream synchronisation; row tables built once, uploaded by every call",
                      "visit": "one child process on one tree's library: corpus built, the four points interleaved, median of `reps`",
                      "order": "parent, this, parent, this, ... per section",
                      "bar": "this tree's median <= the parent's median + the parent's visit-to-visit spread (max - min)"},
           "points": {"short": "1024 queries, one 256-row list each, *_rows_scan 1", "long_off": "one 524288-row list, 16 queries, *_rows_scan 0",
                      "long_scan": "the same list, *_rows_scan 2", "hand_back": "4 overlapping 131072-row lists, 16 queries, *_rows_scan 1"},
           "sections": {}}
    failed = False
    with tempfile.TemporaryDirectory() as tmp:
        for sec in SECTIONS:
            visits = {t: [] for t in trees}
            for v in range(args.visits):
                for t, root in trees.items():
                    part = os.path.join(tmp, f"{sec}_{t}_{v}.json")
                    cmd = [sys.executable, os.path.abspath(__file__), "--section", sec, "--tree", root, "--part", part, "--rows", str(args.rows),
                           "--vocab", str(args.vocab), "--dim", str(args.dim), "--reps", str(args.reps), "--min-seconds", str(args.min_seconds)]
                    try:
                        rc = subprocess.run(cmd, timeout=LIMIT_S, cwd=root).returncode
                    except subprocess.TimeoutExpired:
                        rc = 124
                    if rc != 0:
                        rec["sections"][sec] = f"failed: {t} tree, visit {v}, exit status {rc}"
                        failed = True
                        break                                                # nothing more is started on the device after a failure
                    with open(part) as f:
                        visits[t].append(json.load(f))
                    print(f"[{sec}] visit {v} {t}: " + ", ".join(f"{p} {visits[t][-1][p]['median_ms']:.3f}" for p in POINTS), file=sys.stderr, flush=True)
                if failed:
                    break
            if failed:
                break
            out = {}
            for p in POINTS:
                out[p] = {}
                for t in trees:
                    ms = [vis[p]["median_ms"] for vis in visits[t]]
                    out[p][t] = {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "spread_ms": max(ms) - min(ms),
                                 "visit_medians_ms": ms, "moved": visits[t][-1][p]["moved"]}
                out[p]["within_bar"] = out[p]["this"]["median_ms"] <= out[p]["parent"]["median_ms"] + out[p]["parent"]["spread_ms"]
            rec["sections"][sec] = out
    with open(args.out, "w") as f:
        f.write(json.dumps(rec, indent=1) + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
