#!/usr/bin/env python
"""Cost of the sparse route's set filters (erh_bm25_topk_sets) at the headline corpus shape: 1M documents in four contiguous dir blocks (the
reference's loader walks one directory after the other) over a 262144-term vocabulary, 1024 queries with the reference's question lengths,
k = 192, both BM25 variants.

Sections (each one a child process of this script under its own time limit; the first one that fails ends the run):
  bm25s, okapi   the sparse route alone.  Arms: (i) unfiltered, (ii) one dir per query through the class column, (iii) MatchAny of 2 of the 4
                 dirs and (iv) must_not of 1 of the 4 dirs through erh_bm25_topk_sets, and (iii) / (iv) through erh_bm25_topk_rows with the
                 filter resolved to row lists on the host -- the only exact route without the entry.  The row tables are built once per arm
                 (the host resolution itself is not what is timed); validation, upload and launches of every call are.  Besides the arms: the
                 merge kernel's time per call (event timing, a pass of its own) and the call's sub-query count
  hybrid         bm25s + the dense route (1M x 1024 chunks, k = 288) + RRF top 10 on device lists, both routes on (iii) and on (iv):
                 erh_bm25_topk_sets + erh_dense_topk_sets + erh_dense_check + erh_rrf + one synchronisation, against the same composition with
                 the sparse leg unfiltered (what a fused call under a set filter ran before: two populations)
Arms of a section are interleaved (a b c | c b a | ...; visit 0 is a warm-up that sizes the visits), each arm gets >= --min-seconds of timed
work over --reps visits, every step ends with a stream synchronisation; the report is the median / min / max ms per step.  No thresholds: the
record says what was found.

  python scripts/bm25_sets_timing.py [--sections bm25s,okapi,hybrid] [--out profiles/bm25_sets_timing.json]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from rows_timing import timed  # noqa: E402  (the interleaved-visits timer of the dense script)

SECTIONS = ("bm25s", "okapi", "hybrid")
LIMIT_S = {"bm25s": 300, "okapi": 300, "hybrid": 300}


def section(args):
    import torch
    from easyrag_amd import _lib, synth
    from easyrag_amd.engine import RetrievalEngine, queries_to_csr
    from easyrag_amd.index import BM25S, OKAPI, build_bm25_index_from_postings
    dev = torch.device("cuda", 0)
    n, vocab, k, B, D = args.docs, args.vocab, args.k, args.batch, args.dirs
    eng = RetrievalEngine(0)
    indptr, doc, tf, lens, flat = synth.token_csr_torch(n, vocab, seed=3, device=dev)
    variant = OKAPI if args.section == "okapi" else BM25S
    eng.set_bm25(build_bm25_index_from_postings(indptr, doc, tf, lens, variant, compute_payload=False), payload_on_device=True)
    q = queries_to_csr(synth.token_queries(flat, lens, vocab, B, seed=2000, lengths=synth.REF_QUESTION_LENGTHS))
    del indptr, doc, tf, flat
    dir_id = (np.arange(n) * D // n).astype(np.int16)
    eng.set_doc_meta(n, None, dir_id)
    sync = torch.cuda.synchronize
    one = (np.arange(B) % D).astype(np.int16)
    any2 = [[b % D, (b + 1) % D] for b in range(B)]
    not1 = [[c for c in range(D) if c != b % D] for b in range(B)]
    rec = {}

    def sub_queries(fn, sets):
        before = eng.stat("bm25_sets_subqueries")
        fn()
        return eng.stat("bm25_sets_subqueries") - before

    if args.section != "hybrid":
        # the sets as row lists: one list per distinct set, resolved once
        def tables(sets):
            keys = sorted({tuple(sorted(s)) for s in sets})
            lists = [np.flatnonzero(np.isin(dir_id, np.asarray(key, np.int16))).astype(np.int64) for key in keys]
            lo = np.asarray([keys.index(tuple(sorted(s))) for s in sets], np.int32)
            return RetrievalEngine.lists_to_csr(lists, lo, B)
        tabs = {"iii_rows": tables(any2), "iv_rows": tables(not1)}
        sets = {"iii_sets": any2, "iv_sets": not1}

        def step(arm):
            if arm == "i":
                out = eng.bm25_topk(*q, k, device_out=True)
            elif arm == "ii":
                out = eng.bm25_topk(*q, k, filter_dir=one, device_out=True)
            elif arm in sets:
                out = eng.bm25_topk_sets(*q, k, sets[arm], device_out=True)
            else:
                out = eng.bm25_topk_rows_csr(*q, k, *tabs[arm], device_out=True)
            eng.sync()
            return out
        # two groups, each interleaved: the scans, and the rows arms (hundreds of thousands of listed rows per query: one step per visit)
        rec["arms"] = timed(["i", "ii", "iii_sets", "iv_sets"], step, sync, args.steps, args.reps, args.min_seconds)
        rec["arms"].update(timed(["iii_rows", "iv_rows"], step, sync, 1, args.reps, 0.0))
        print(f"[{args.section}] " + ", ".join(f"{a} {v['median_ms']:.3f} ms" for a, v in rec["arms"].items()), file=sys.stderr, flush=True)
        # the merge kernel alone: event timing of its class over a few calls (at >= 512 sub-queries the scans run one segment per query, so
        # nothing else books to the class)
        eng.set_profiling(True)
        for arm in sets:
            eng.reset_kernel_time()
            n_sub = 0
            for _ in range(5):
                n_sub = sub_queries(lambda: step(arm), sets[arm])
            t = eng.kernel_time(_lib.ERH_K_BM25_MERGE)
            s = eng.kernel_time(_lib.ERH_K_BM25_SCAN)
            rec[arm] = {"bm25_sets_subqueries_per_call": n_sub, "merge_ms_per_call": t["ms"] / 5, "merge_launches_per_call": t["launches"] / 5,
                        "scan_ms_per_call": s["ms"] / 5, "scan_launches_per_call": s["launches"] / 5}
        eng.set_profiling(False)
    else:
        d, kd = args.dim, 288
        x = synth.dense_corpus_torch(n, d, seed=2, device=dev)
        eng.set_dense(x)
        emb = synth.dense_queries_torch(x, B, seed=1000)
        both = {"iii": any2, "iv": not1}

        def step(arm):
            which, sparse = arm.split("_")
            if sparse == "sets":
                sids, _, sln = eng.bm25_topk_sets(*q, k, both[which], device_out=True)
            else:
                sids, _, sln = eng.bm25_topk(*q, k, device_out=True)
            dids, _, dln = eng.dense_topk_sets(emb, kd, both[which], device_out=True)
            eng.dense_check()
            out = eng.rrf_device(sids, sln, dids, dln, K=60, topk=10)
            eng.sync()
            return out
        arms = ["iii_sets", "iii_unfiltered", "iv_sets", "iv_unfiltered"]
        rec["arms"] = timed(arms, step, sync, args.steps, args.reps, args.min_seconds)
        print(f"[{args.section}] " + ", ".join(f"{a} {v['median_ms']:.3f} ms" for a, v in rec["arms"].items()), file=sys.stderr, flush=True)
    rec["stats"] = eng.stats()
    eng.close()
    with open(args.part, "w") as f:
        json.dump(rec, f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--vocab", type=int, default=262_144)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--dirs", type=int, default=4)
    ap.add_argument("--k", type=int, default=192)
    ap.add_argument("--sections", default=",".join(SECTIONS))
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--min-seconds", type=float, default=0.3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bm25_sets_timing.json"))
    ap.add_argument("--section", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--part", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.section:
        return section(args)
    rec = {"shape": {"docs": args.docs, "vocab": args.vocab, "dirs": args.dirs, "layout": "contiguous blocks", "batch": args.batch, "k": args.k,
                     "query_lengths": "the reference's 103 questions", "hybrid": {"dim": args.dim, "k_dense": 288, "topk": 10}},
           "method": {"reps": args.reps, "min_seconds": args.min_seconds, "every step": "device outputs + one stream synchronisation",
                      "rows arms": "erh_bm25_topk_rows on row tables resolved once on the host, uploaded by every call"}, "sections": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for sec in [s for s in args.sections.split(",") if s]:
            part = os.path.join(tmp, sec + ".json")
            cmd = [sys.executable, os.path.abspath(__file__), "--section", sec, "--part", part, "--docs", str(args.docs), "--vocab", str(args.vocab),
                   "--dim", str(args.dim), "--batch", str(args.batch), "--dirs", str(args.dirs), "--k", str(args.k), "--steps", str(args.steps),
                   "--reps", str(args.reps), "--min-seconds", str(args.min_seconds)]
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
    print(txt)
    with open(args.out, "w") as f:
        f.write(txt + "\n")
    return 0 if all(isinstance(v, dict) for v in rec["sections"].values()) else 1


if __name__ == "__main__":
    sys.exit(main())
