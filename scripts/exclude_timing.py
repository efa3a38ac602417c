#!/usr/bin/env python
"""Cost of the exclude lists (erh_dense_topk_excl / erh_bm25_topk_excl, DESIGN K12) at the headline corpus shape: 1M x 1024 chunks, k = 288
on the dense route; 1M documents over a 262144-term vocabulary, the reference's question lengths, k = 192 on the sparse route (bm25s); the
hybrid = both + RRF top 10 on device lists.  Batches of 1024 queries and of one query.

Sections (each one a child process of this script under its own time limit; the first one that fails ends the run):
  dense, sparse  per batch size, interleaved: `plain` -- the same call without exclusion (erh_dense_topk + erh_dense_check / erh_bm25_topk) --,
                 `excl_e` for e in 0, 10, 100, 480 ids per query (the query's own best e ids of a deeper plain call, what paging excludes:
                 every one of them is really dropped), and `complement_e10`: the only device route without the entries, every row but
                 the e excluded ones as a rows= list.  One query: its own list of N - 10 rows (4 MB validated and uploaded per call).
                 1024 queries: ONE list shared by all of them (every query excludes the same 10 ids) -- the complement's best case; one
                 list per query would be 4 GB of ids per call and is not run.
  hybrid         erh_bm25_topk_excl + erh_dense_topk_excl + erh_rrf + one synchronisation for the same e, against erh_bm25_topk +
                 erh_dense_topk + erh_dense_check + erh_rrf.
Arms are interleaved (a b c | c b a | ...; visit 0 is a warm-up that sizes the visits), each arm gets >= --min-seconds of timed work over
--reps visits, every step ends with a stream synchronisation; the report is the median / min / max ms per step.  No thresholds: the record
says what was found.

  python scripts/exclude_timing.py [--sections dense,sparse,hybrid] [--out profiles/exclude_timing.json]
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

SECTIONS = ("dense", "sparse", "hybrid")
LIMIT_S = {"dense": 300, "sparse": 300, "hybrid": 300}
ES = (0, 10, 100, 480)


def section(args):
    import torch
    from easyrag_amd import synth
    from easyrag_amd.engine import RetrievalEngine, queries_to_csr
    from easyrag_amd.index import BM25S, build_bm25_index_from_postings
    dev = torch.device("cuda", 0)
    n, B = args.docs, args.batch
    kd, ks = 288, 192
    eng = RetrievalEngine(0)
    sync = torch.cuda.synchronize
    sec = args.section
    if sec in ("dense", "hybrid"):
        x = synth.dense_corpus_torch(n, args.dim, seed=2, device=dev)
        eng.set_dense(x)
        emb = synth.dense_queries_torch(x, B, seed=1000)
    if sec in ("sparse", "hybrid"):
        indptr, doc, tf, lens, flat = synth.token_csr_torch(n, args.vocab, seed=3, device=dev)
        eng.set_bm25(build_bm25_index_from_postings(indptr, doc, tf, lens, BM25S, compute_payload=False), payload_on_device=True)
        qs = synth.token_queries(flat, lens, args.vocab, B, seed=2000, lengths=synth.REF_QUESTION_LENGTHS)
        del indptr, doc, tf, flat
    # what a query excludes: its own best ids of a deeper plain call (the dense route's where there is one)
    if sec == "sparse":
        deep = eng.bm25_topk(*queries_to_csr(qs), 1024)
    else:
        deep = eng.dense_topk(emb, 768)
    top = np.asarray(deep[0])
    excl_of = {e: [np.sort(top[b, :e][top[b, :e] >= 0]) for b in range(B)] for e in ES}
    rec = {}
    for nb in (B, 1):
        sub = slice(0, nb)
        ex = {e: RetrievalEngine.excl_to_csr(excl_of[e][sub], nb) for e in ES}
        q = queries_to_csr(qs[sub]) if sec != "dense" else None
        qe = emb[sub] if sec != "sparse" else None
        lists = None
        if sec != "hybrid":
            gone = excl_of[10][0]
            shared = np.setdiff1d(np.arange(n, dtype=np.int64), gone)
            lists = RetrievalEngine.lists_to_csr([shared], np.zeros(nb, np.int32), nb)

        def excl_call(route, e, **kw):
            if route == "dense":                        # (the tables are built once: what is timed is the entry)
                return eng.dense_topk_excl_csr(qe, kd, *ex[e], device_out=True, **kw)
            return eng.bm25_topk_excl_csr(*q, ks, *ex[e], device_out=True, **kw)

        def step(arm):
            if sec == "hybrid":
                if arm == "plain":
                    sids, _, sln = eng.bm25_topk(*q, ks, device_out=True)
                    dids, _, dln = eng.dense_topk(qe, kd, device_out=True)
                    eng.dense_check()
                else:
                    e = int(arm.split("_e")[1])
                    sids, _, sln = excl_call("sparse", e)
                    dids, _, dln = excl_call("dense", e)
                out = eng.rrf_device(sids, sln, dids, dln, K=60, topk=10)
            elif arm == "plain":
                if sec == "dense":
                    out = eng.dense_topk(qe, kd, device_out=True)
                    eng.dense_check()
                else:
                    out = eng.bm25_topk(*q, ks, device_out=True)
            elif arm.startswith("excl_e"):
                out = excl_call(sec, int(arm.split("_e")[1]))
            elif sec == "dense":
                out = eng.dense_topk_rows_csr(qe, kd, *lists, device_out=True)
            else:
                out = eng.bm25_topk_rows_csr(*q, ks, *lists, device_out=True)
            eng.sync()
            return out
        arms = ["plain"] + [f"excl_e{e}" for e in ES]
        got = timed(arms, step, sync, args.steps, args.reps, args.min_seconds)
        if sec != "hybrid":
            got.update(timed(["complement_e10"], step, sync, 1, args.reps, 0.0))
        rec[f"batch_{nb}"] = got
        print(f"[{sec} x {nb}] " + ", ".join(f"{a} {v['median_ms']:.3f} ms" for a, v in got.items()), file=sys.stderr, flush=True)
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
    ap.add_argument("--sections", default=",".join(SECTIONS))
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--min-seconds", type=float, default=0.3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exclude_timing.json"))
    ap.add_argument("--section", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--part", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.section:
        return section(args)
    rec = {"shape": {"docs": args.docs, "vocab": args.vocab, "dim": args.dim, "batch": [args.batch, 1], "k_dense": 288, "k_sparse": 192,
                     "variant": "bm25s", "query_lengths": "the reference's 103 questions", "hybrid_topk": 10, "excluded_per_query": list(ES)},
           "method": {"reps": args.reps, "min_seconds": args.min_seconds, "every step": "device outputs + one stream synchronisation",
                      "excluded ids": "the query's own best e ids of a deeper plain call, so every one of them is dropped",
                      "complement_e10": "erh_*_topk_rows over every row but the 10 excluded ones, tables built once, validated and uploaded "
                                        "by every call; 1024 queries share ONE list (the complement's best case), one query has its own"},
           "sections": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for sec in [s for s in args.sections.split(",") if s]:
            part = os.path.join(tmp, sec + ".json")
            cmd = [sys.executable, os.path.abspath(__file__), "--section", sec, "--part", part, "--docs", str(args.docs), "--vocab", str(args.vocab),
                   "--dim", str(args.dim), "--batch", str(args.batch), "--steps", str(args.steps), "--reps", str(args.reps),
                   "--min-seconds", str(args.min_seconds)]
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
