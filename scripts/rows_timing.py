#!/usr/bin/env python
"""Cost of the dense route over explicit row lists (erh_dense_topk_rows) against the route the same query takes without it -- the class
column of erh_dense_topk, dir blocks as configured by default -- at the headline corpus shape, 1M x 1024 chunks.

Sections (each one a child process of this script under its own time limit; the first one that fails ends the run):
  single   one filtered query per call on a class of 200 / 1000 / 4000 rows: column vs rows
  batch    1024 queries, each on its own 200-row dir out of 5000: column vs rows; then a corpus of 40000 dirs of 25 rows -- more classes than
           the int16 class column numbers, which the retrievers used to refuse with a ValueError -- through rows alone
  sweep    list length 256 ... N/2 at 1, 64 and 1024 queries; `shared`: every query on the same class; `distinct`: query b on class
           b mod (N / length) of a corpus cut into classes of that length.  Points with more than --max-row-scores (query, row) pairs are
           skipped and recorded as such.  `crossover` = per (queries, layout) the first length at which the rows entry is no longer faster.
Arms of a comparison are interleaved (a b | b a | ...; visit 0 is a warm-up that sizes the visits), each arm gets >= --min-seconds of timed
work over --reps visits, every step of the column route ends with erh_dense_check and every rows step with a stream synchronisation (what
a caller of device outputs must do); the report is the median / min / max ms per step.

  python scripts/rows_timing.py [--sections single,batch,sweep] [--out profiles/dense_rows_timing.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SECTIONS = ("single", "batch", "sweep")
# the entry's fixed choices (csrc/kernels.h: kDenseRowsShortMax, kDenseRowsGroup, kDenseRowsSeg; option dense_rows_ws_mb), recorded with the figures
ROWS_CHOICES = {"short_shape_max_rows": 2048, "long_shape_queries_per_group": 8, "long_shape_rows_per_segment": 1024, "work_space_mb": 256}
LIMIT_S = {"single": 240, "batch": 300, "sweep": 600}


def timed(arms, step, sync, steps0, reps, min_seconds):
    """arms: names; step(name) runs one step.  Interleaved visits, median of `reps`."""
    ms = {a: [] for a in arms}
    steps = {a: steps0 for a in arms}
    for rep in range(reps + 1):
        for arm in (arms if rep % 2 == 0 else arms[::-1]):
            step(arm)
            sync()
            t0 = time.perf_counter()
            for _ in range(steps[arm]):
                step(arm)
            sync()
            dt = time.perf_counter() - t0
            if rep == 0:
                steps[arm] = max(steps0, int(np.ceil(min_seconds / reps / (dt / steps[arm]))))
                continue
            ms[arm].append(dt / steps[arm] * 1e3)
    return {a: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "visits": len(v), "steps_per_visit": steps[a]}
            for a, v in ms.items()}


def section(args):
    import torch
    from easyrag_amd import synth
    from easyrag_amd.engine import RetrievalEngine
    dev = torch.device("cuda", 0)
    n, d, k = args.chunks, args.dim, args.k
    eng = RetrievalEngine(0)
    # the `rows` arms here are the row-by-row shapes: the scan route of long lists (DESIGN K11) is off unless asked for -- its own sweep,
    # both arms interleaved, is scripts/rows_scan_timing.py
    eng.set_option("dense_rows_scan", args.rows_scan)
    x = synth.dense_corpus_torch(n, d, seed=2, device=dev)
    eng.set_dense(x)
    qall = synth.dense_queries_torch(x, 1024, seed=1000)
    sync = torch.cuda.synchronize
    rec = {}

    def column(q, col):
        out = eng.dense_topk(q, k, filter_dir=col, device_out=True)
        eng.dense_check()
        return out

    csr = {}

    def rows(q, lists, lo):
        # the C entry's tables are built once per arm (the Python list handling is not what is timed); validation, table upload and
        # launches of every call are
        key = id(lists)
        if key not in csr:
            csr.clear()
            csr[key] = (lists, RetrievalEngine.lists_to_csr(lists, lo, q.shape[0]))
        out = eng.dense_topk_rows_csr(q, k, *csr[key][1], device_out=True)
        eng.sync()
        return out

    def compare(q, col, lists, lo):
        def step(arm):
            return column(q, col) if arm == "column" else rows(q, lists, lo)
        return timed(["column", "rows"], step, sync, args.steps, args.reps, args.min_seconds)

    if args.section == "single":
        sizes = (200, 1000, 4000)
        dir_id = np.full(n, 3, np.int16)
        lists = []
        for c, sz in enumerate(sizes):
            at = 100_000 * (c + 1)
            dir_id[at:at + sz] = c
            lists.append(np.arange(at, at + sz, dtype=np.int64))
        eng.set_doc_meta(n, None, dir_id)
        q = qall[:1]
        for c, sz in enumerate(sizes):
            rec[f"class_{sz}"] = compare(q, np.asarray([c], np.int16), [lists[c]], np.zeros(1, np.int32))
    elif args.section == "batch":
        B = 1024
        rng = np.random.default_rng(5)
        dir_id = (np.arange(n) // 200).astype(np.int16)                      # 5000 dirs of 200 rows
        eng.set_doc_meta(n, None, dir_id)
        dirs = rng.choice(n // 200, size=B, replace=False)
        lists = [np.arange(200 * c, 200 * c + 200, dtype=np.int64) for c in dirs]
        rec["dirs_5000_x_200"] = compare(qall, dirs.astype(np.int16), lists, np.arange(B, dtype=np.int32))
        dirs = rng.choice(n // 25, size=B, replace=False)                     # 40000 dirs of 25 rows: no class column can hold them
        lists = [np.arange(25 * c, 25 * c + 25, dtype=np.int64) for c in dirs]
        eng.set_doc_meta(n, None, None)
        r = timed(["rows"], lambda arm: rows(qall, lists, np.arange(B, dtype=np.int32)), sync, args.steps, args.reps, args.min_seconds)
        rec["dirs_40000_x_25"] = {"rows": r["rows"], "column": "not possible: more than 32000 classes (a ValueError before this entry existed)"}
    else:
        lengths = [L for L in (256, 1024, 4096, 16384, 65536, 262144, n // 2) if L <= n // 2]
        cross = {}
        for L in lengths:
            n_cls = n // L
            dir_id = np.minimum(np.arange(n) // L, n_cls - 1).astype(np.int16)
            eng.set_doc_meta(n, None, dir_id)
            for B in (1, 64, 1024):
                q = qall[:B]
                for layout in ("shared", "distinct"):
                    name = f"len_{L}_q_{B}_{layout}"
                    if B * L > args.max_row_scores:
                        rec[name] = "skipped: more (query, row) pairs than --max-row-scores"
                        continue
                    cls = np.zeros(B, np.int64) if layout == "shared" else np.arange(B) % n_cls
                    uniq = np.unique(cls)
                    lists = [np.flatnonzero(dir_id == c).astype(np.int64) for c in uniq]
                    lo = np.searchsorted(uniq, cls).astype(np.int32)
                    r = rec[name] = compare(q, cls.astype(np.int16), lists, lo)
                    key = f"q_{B}_{layout}"
                    if key not in cross and r["rows"]["median_ms"] >= r["column"]["median_ms"]:
                        cross[key] = L
        rec["crossover"] = {f"q_{B}_{layout}": cross.get(f"q_{B}_{layout}", "none up to the longest length measured")
                            for B in (1, 64, 1024) for layout in ("shared", "distinct")}
    rec["stats"] = eng.stats()
    eng.close()
    with open(args.part, "w") as f:
        json.dump(rec, f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--k", type=int, default=288)
    ap.add_argument("--sections", default=",".join(SECTIONS))
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--min-seconds", type=float, default=0.3)
    ap.add_argument("--max-row-scores", type=int, default=1 << 26)
    ap.add_argument("--rows-scan", type=int, default=0, choices=(0, 1, 2),
                    help="option dense_rows_scan for every rows arm: 0 = the row-by-row shapes (default), 1 = by the work rule, 2 = every long list")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_rows_timing.json"))
    ap.add_argument("--section", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--part", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.section:
        return section(args)
    rec = {"shape": {"chunks": args.chunks, "dim": args.dim, "k": args.k},
           "options": {"dense_rows_scan": args.rows_scan, "note": "the `rows` arms ran with this value; a default handle has 1 (lists of at least "
                       "dense_rows_scan_min_rows rows go through the scan where the work rule says so: scripts/rows_scan_timing.py)"},
           "choices": ROWS_CHOICES,
           "method": {"reps": args.reps, "min_seconds": args.min_seconds, "column": "erh_dense_topk + erh_dense_check, default options",
                      "rows": "erh_dense_topk_rows + erh_sync, tables uploaded by every call"}, "sections": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for sec in [s for s in args.sections.split(",") if s]:
            part = os.path.join(tmp, sec + ".json")
            cmd = [sys.executable, os.path.abspath(__file__), "--section", sec, "--part", part, "--chunks", str(args.chunks), "--dim", str(args.dim),
                   "--k", str(args.k), "--steps", str(args.steps), "--reps", str(args.reps), "--min-seconds", str(args.min_seconds),
                   "--max-row-scores", str(args.max_row_scores), "--rows-scan", str(args.rows_scan)]
            try:
                rc = subprocess.run(cmd, timeout=LIMIT_S[sec]).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:
                rec["sections"][sec] = f"failed: exit status {rc}"
                break                                                        # nothing more is started on the device after a failure
            with open(part) as f:
                rec["sections"][sec] = json.load(f)
    txt = json.dumps(rec, indent=1)
    print(txt)
    with open(args.out, "w") as f:
        f.write(txt + "\n")
    return 0 if all(isinstance(v, dict) for v in rec["sections"].values()) else 1


if __name__ == "__main__":
    sys.exit(main())
