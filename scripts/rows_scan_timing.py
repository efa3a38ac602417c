#!/usr/bin/env python
"""Long row lists through the scan (DESIGN K11): where erh_dense_topk_rows / erh_bm25_topk_rows on a call-local class column beat the
row-by-row shapes, at the headline corpus shape (1M rows; dense d = 1024, k = 100; BM25 over a 262144-term vocabulary, the reference's
question lengths, k = 192).

Sections (each one a child process under its own time limit; the first one that fails ends the run):
  dense, bm25s, okapi   the sweep: list length x queries per call x {one shared list, 4 overlapping lists}, the arms `rows` (option
                        *_rows_scan = 0: the shapes every rows call took before the route existed, same kernels), `scan` (= 2: every list
                        routed) and `rule` (= 1, the default: what a call costs when the work rule decides, the classification it throws
                        away where it says no included), interleaved; and which arm the rule takes at the point.  Then the host share of a routed call
                        (validation alone -- a call refused at its last row --, and wall time minus the kernels' event time).
  bm25s, okapi also     the two rows arms of scripts/bm25_sets_timing.py again (MatchAny of 2 of 4 dirs, must_not of 1 of 4 dirs as row lists,
                        1024 queries) beside their class-set arms, with the route off and by the rule.
The rule's constants are fitted from the sweep by hand (every point records both arms with their spread and the arm the rule takes: the
constants are right when that is the faster one, or the two are within the spread); no thresholds here: the record says what was found.

  python scripts/rows_scan_timing.py [--sections dense,bm25s,okapi] [--out profiles/rows_scan_timing.json]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from rows_timing import timed  # noqa: E402  (the interleaved-visits timer of the dense script)

SECTIONS = ("dense", "bm25s", "okapi")
LIMIT_S = {"dense": 420, "bm25s": 420, "okapi": 420}
LENGTHS = (131072, 262144, 524288, -1)                                       # -1: N - 1
BATCHES = (1, 16, 256, 1024)


def section(args):
    import torch
    from easyrag_amd import _lib, synth
    from easyrag_amd.engine import RetrievalEngine, queries_to_csr
    from easyrag_amd.index import BM25S, OKAPI, build_bm25_index_from_postings
    dev = torch.device("cuda", 0)
    n = args.rows
    dense = args.section == "dense"
    route = "dense" if dense else "bm25"
    eng = RetrievalEngine(0)
    sync = torch.cuda.synchronize
    if dense:
        k = 100
        x = synth.dense_corpus_torch(n, args.dim, seed=2, device=dev)
        eng.set_dense(x)
        qall = synth.dense_queries_torch(x, max(BATCHES), seed=1000)

        def call(B, csr):
            return eng.dense_topk_rows_csr(qall[:B], k, *csr, device_out=True)
    else:
        k = 192
        indptr, doc, tf, lens, flat = synth.token_csr_torch(n, args.vocab, seed=3, device=dev)
        variant = OKAPI if args.section == "okapi" else BM25S
        eng.set_bm25(build_bm25_index_from_postings(indptr, doc, tf, lens, variant, compute_payload=False), payload_on_device=True)
        queries = synth.token_queries(flat, lens, args.vocab, max(BATCHES), seed=2000, lengths=synth.REF_QUESTION_LENGTHS)
        qcsr = {B: queries_to_csr(queries[:B]) for B in BATCHES}
        del indptr, doc, tf, flat

        def call(B, csr):
            return eng.bm25_topk_rows_csr(*qcsr[B], k, *csr, device_out=True)

    rng = np.random.default_rng(5)
    rec = {"k": k, "sweep": [], "options": {o: eng.get_option(o) for o in
                                             ([route + "_rows_scan_gain", route + "_rows_scan_min_rows"] +
                                              (["dense_route_ridge", "dense_rows_scan_small_cell"] if dense else ["bm25_rows_scan_floor"]))}}
    for L in LENGTHS:
        length = n - 1 if L < 0 else L
        for layout in ("one list", "4 overlapping lists"):
            if layout == "one list":
                lists = [np.sort(rng.choice(n, size=length, replace=False)).astype(np.int64)]
            else:
                lists = [np.sort(rng.choice(n, size=length, replace=False)).astype(np.int64) for _ in range(4)]
            for B in BATCHES:
                lo = (np.arange(B) % len(lists)).astype(np.int32)
                csr = RetrievalEngine.lists_to_csr(lists, lo, B)

                def step(arm):
                    eng.set_option(route + "_rows_scan", {"rows": 0, "rule": 1, "scan": 2}[arm])
                    out = call(B, csr)
                    eng.sync()
                    return out
                t = timed(["rows", "scan", "rule"], step, sync, 1, args.reps, args.min_seconds)
                eng.set_option(route + "_rows_scan", 1)
                before = (eng.stat(route + "_rows_scan_calls"), eng.stat(route + "_rows_scan_subqueries"))
                call(B, csr)
                eng.sync()
                took = eng.stat(route + "_rows_scan_calls") - before[0]
                point = {"length": length, "layout": layout, "queries": B, "rows_ms": t["rows"], "scan_ms": t["scan"], "rule_ms": t["rule"],
                         "rule_takes": "scan" if took else "rows"}
                eng.set_option(route + "_rows_scan", 2)
                before = eng.stat(route + "_rows_scan_subqueries")
                call(B, csr)
                eng.sync()
                point["sub_queries"] = eng.stat(route + "_rows_scan_subqueries") - before
                rec["sweep"].append(point)
                print(f"[{args.section}] {length} x {B} ({layout}): rows {t['rows']['median_ms']:.3f} ms, scan {t['scan']['median_ms']:.3f} ms, "
                      f"rule {t['rule']['median_ms']:.3f} ms, takes {point['rule_takes']}", file=sys.stderr, flush=True)
    # the host share of a routed call: 1024 queries on one 524288-row list
    B, length = 1024, 524288
    lists = [np.sort(rng.choice(n, size=length, replace=False)).astype(np.int64)]
    csr = RetrievalEngine.lists_to_csr(lists, np.zeros(B, np.int32), B)
    eng.set_option(route + "_rows_scan", 2)
    call(B, csr)
    eng.sync()
    eng.set_profiling(True)
    eng.reset_kernel_time()
    t0 = time.perf_counter()
    for _ in range(5):
        call(B, csr)
        eng.sync()
    wall = (time.perf_counter() - t0) / 5 * 1e3
    kern = sum(eng.kernel_time(c)["ms"] for c in range(6)) / 5
    eng.set_profiling(False)
    bad = (csr[0], csr[1].copy(), csr[2])
    bad[1][-1] = n                                                            # refused at the last row: the validation alone
    t0 = time.perf_counter()
    for _ in range(5):
        try:
            call(B, bad)
        except _lib.ErhError:
            pass
    valid = (time.perf_counter() - t0) / 5 * 1e3
    rec["host_share"] = {"queries": B, "length": length, "wall_ms": wall, "kernel_event_ms": kern, "validation_ms": valid,
                         "list_bytes": int(csr[1].nbytes), "note": "wall - kernel events = validation + table build + upload + launches + the "
                         "read-back of the cells; python call overhead included"}
    if not dense:
        # the rows arms of scripts/bm25_sets_timing.py: 4 contiguous dirs, MatchAny of 2 / must_not of 1 as row lists, beside the class sets
        D, B = 4, 1024
        dir_id = (np.arange(n) * D // n).astype(np.int16)
        eng.set_doc_meta(n, None, dir_id)
        any2 = [[b % D, (b + 1) % D] for b in range(B)]
        not1 = [[c for c in range(D) if c != b % D] for b in range(B)]

        def tables(sets):
            keys = sorted({tuple(sorted(s)) for s in sets})
            lists = [np.flatnonzero(np.isin(dir_id, np.asarray(key, np.int16))).astype(np.int64) for key in keys]
            lo = np.asarray([keys.index(tuple(sorted(s))) for s in sets], np.int32)
            return RetrievalEngine.lists_to_csr(lists, lo, B)
        tabs = {"iii": tables(any2), "iv": tables(not1)}
        sets = {"iii": any2, "iv": not1}

        def step(arm):
            which, how = arm.split("_", 1)
            if how == "sets":
                out = eng.bm25_topk_sets(*qcsr[B], k, sets[which], device_out=True)
            else:
                eng.set_option("bm25_rows_scan", 0 if how == "rows_off" else 1)
                out = eng.bm25_topk_rows_csr(*qcsr[B], k, *tabs[which], device_out=True)
            eng.sync()
            return out
        rec["sets_timing_arms"] = timed(["iii_sets", "iii_rows_rule", "iv_sets", "iv_rows_rule"], step, sync, 2, args.reps, args.min_seconds)
        rec["sets_timing_arms"].update(timed(["iii_rows_off", "iv_rows_off"], step, sync, 1, args.reps, 0.0))
        eng.set_option("bm25_rows_scan", 1)
        before = eng.stat("bm25_rows_scan_calls")
        step("iii_rows_rule")
        step("iv_rows_rule")
        rec["sets_timing_arms"]["rule_routed_calls_of_2"] = eng.stat("bm25_rows_scan_calls") - before
        print(f"[{args.section}] " + ", ".join(f"{a} {v['median_ms']:.3f} ms" for a, v in rec["sets_timing_arms"].items() if isinstance(v, dict)),
              file=sys.stderr, flush=True)
    rec["stats"] = eng.stats()
    eng.close()
    with open(args.part, "w") as f:
        json.dump(rec, f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--vocab", type=int, default=262_144)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--sections", default=",".join(SECTIONS))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--min-seconds", type=float, default=0.1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rows_scan_timing.json"))
    ap.add_argument("--section", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--part", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.section:
        return section(args)
    rec = {"shape": {"rows": args.rows, "dense": {"dim": args.dim, "k": 100}, "bm25": {"vocab": args.vocab, "k": 192,
                                                                                        "query_lengths": "the reference's 103 questions"}},
           "method": {"reps": args.reps, "min_seconds": args.min_seconds, "every step": "device outputs + one stream synchronisation",
                      "arms": "rows = *_rows_scan 0 (the row-by-row shapes, the only path before the route), scan = 2, rule = 1 (the default); "
                              "interleaved visits, "
                              "median / min / max ms per call; row tables built once, uploaded by every call"}, "sections": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for sec in [s for s in args.sections.split(",") if s]:
            part = os.path.join(tmp, sec + ".json")
            cmd = [sys.executable, os.path.abspath(__file__), "--section", sec, "--part", part, "--rows", str(args.rows), "--vocab", str(args.vocab),
                   "--dim", str(args.dim), "--reps", str(args.reps), "--min-seconds", str(args.min_seconds)]
            try:
                rc = subprocess.run(cmd, timeout=LIMIT_S[sec]).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:
                rec["sections"][sec] = f"failed: exit status {rc}"
                break                                                        # nothing more is started on the device after a failure
            with open(part) as f:
                rec["sections"][sec] = json.load(f)
            with open(args.out, "w") as f:                                   # (after every section: a run cut short keeps what it has)
                f.write(json.dumps(rec, indent=1) + "\n")
    txt = json.dumps(rec, indent=1)
    with open(args.out, "w") as f:
        f.write(txt + "\n")
    return 0 if all(isinstance(v, dict) for v in rec["sections"].values()) else 1


if __name__ == "__main__":
    sys.exit(main())
