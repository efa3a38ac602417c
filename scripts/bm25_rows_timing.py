#!/usr/bin/env python
"""Cost of the sparse route over explicit row lists (erh_bm25_topk_rows) against what the same question costs without it, at the headline
corpus shape: 1M documents over a 262144-term vocabulary, bm25s payloads, queries with the reference's question lengths.

Sections (each one a child process of this script under its own time limit; the first one that fails ends the run):
  single   one query per call on a dir of 200 / 1000 / 4000 rows: the class column of erh_bm25_topk vs rows
  batch    1024 queries, each on its own list of 200 arbitrary rows.  No class column can express that; the only exact route without the entry is
           erh_bm25_scores (one launch per query token, an N-long fp64 vector to the host) plus a host walk, one query at a time.  That arm is
           timed on --walk-queries queries and reported per query and extrapolated to the batch; the rows arm runs the whole batch
  sweep    list length 256 ... N/2 at 1, 64 and 1024 queries, query b on class b mod (N / length) of a corpus cut into classes of that length:
           rows vs the class column vs the unfiltered scan of the whole corpus (`corpus`: what a scan costs whatever the filter).  Points with
           more than --max-row-scores (query, row) pairs are skipped and recorded as such.  `crossover` = per batch size the first length at
           which the rows entry is no longer faster than the class column / than the whole-corpus scan
  hybrid   1024 queries, each on its own 200-row dir, both routes on rows: erh_bm25_topk_rows + erh_dense_topk_rows + erh_rrf on device lists
           + one synchronisation, vs the composition with the sparse leg on the class column (what a fused call over an id set ran before)
Arms of a comparison are interleaved (a b | b a | ...; visit 0 is a warm-up that sizes the visits), each arm gets >= --min-seconds of timed
work over --reps visits, every step ends with a stream synchronisation (what a caller of device outputs must do); the report is the median /
min / max ms per step.

  python scripts/bm25_rows_timing.py [--sections single,batch,sweep,hybrid] [--out profiles/bm25_rows_timing.json]
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

SECTIONS = ("single", "batch", "sweep", "hybrid")
# the entry's fixed choices (csrc/kernels.h: kBm25RowsShortMax, kBm25RowsSeg; option bm25_rows_ws_mb), recorded with the figures
ROWS_CHOICES = {"short_shape_max_rows": 2048, "long_shape_rows_per_segment": 2048, "work_space_mb": 256}
LIMIT_S = {"single": 240, "batch": 300, "sweep": 600, "hybrid": 300}


def section(args):
    import torch
    from easyrag_amd import synth
    from easyrag_amd.engine import RetrievalEngine, queries_to_csr
    from easyrag_amd.index import BM25S, build_bm25_index_from_postings
    dev = torch.device("cuda", 0)
    n, vocab, k = args.docs, args.vocab, args.k
    eng = RetrievalEngine(0)
    # the `rows` arms here are the row-by-row shapes: the scan route of long lists (DESIGN K11) is off unless asked for -- its own sweep,
    # both arms interleaved, is scripts/rows_scan_timing.py
    eng.set_option("bm25_rows_scan", args.rows_scan)
    indptr, doc, tf, lens, flat = synth.token_csr_torch(n, vocab, seed=3, device=dev)
    eng.set_bm25(build_bm25_index_from_postings(indptr, doc, tf, lens, BM25S, compute_payload=False), payload_on_device=True)
    toks = synth.token_queries(flat, lens, vocab, 1024, seed=2000, lengths=synth.REF_QUESTION_LENGTHS)
    del indptr, doc, tf, flat
    sync = torch.cuda.synchronize
    rec = {}
    csr = {}

    def column(q, col):
        out = eng.bm25_topk(*q, k, filter_dir=col, device_out=True)
        eng.sync()
        return out

    def rows(q, lists, lo):
        # the C entry's tables are built once per arm (the Python list handling is not what is timed); validation, table upload and
        # launches of every call are
        key = id(lists)
        if key not in csr:
            csr.clear()
            csr[key] = (lists, RetrievalEngine.lists_to_csr(lists, lo, q[0].shape[0] - 1))
        out = eng.bm25_topk_rows_csr(*q, k, *csr[key][1], device_out=True)
        eng.sync()
        return out

    def compare(q, col, lists, lo, corpus=False):
        def step(arm):
            return rows(q, lists, lo) if arm == "rows" else column(q, col if arm == "column" else None)
        r = timed(["column", "rows"] + (["corpus"] if corpus else []), step, sync, args.steps, args.reps, args.min_seconds)
        print(f"[{args.section}] {q[0].shape[0] - 1} queries, {sum(len(l) for l in lists)} listed rows: "
              + ", ".join(f"{a} {v['median_ms']:.3f} ms" for a, v in r.items()), file=sys.stderr, flush=True)
        return r

    if args.section == "single":
        sizes = (200, 1000, 4000)
        dir_id = np.full(n, 3, np.int16)
        lists = []
        for c, sz in enumerate(sizes):
            at = (n // 10) * (c + 1)
            dir_id[at:at + sz] = c
            lists.append(np.arange(at, at + sz, dtype=np.int64))
        eng.set_doc_meta(n, None, dir_id)
        q = queries_to_csr(toks[:1])
        for c, sz in enumerate(sizes):
            rec[f"dir_{sz}"] = compare(q, np.asarray([c], np.int16), [lists[c]], np.zeros(1, np.int32))
    elif args.section == "batch":
        B = 1024
        rng = np.random.default_rng(5)
        lists = [np.sort(rng.choice(n, size=200, replace=False)).astype(np.int64) for _ in range(B)]
        q = queries_to_csr(toks)
        r = timed(["rows"], lambda arm: rows(q, lists, np.arange(B, dtype=np.int32)), sync, args.steps, args.reps, args.min_seconds)
        W = min(args.walk_queries, B)

        def walk(arm):
            for b in range(W):
                s = eng.bm25_scores(toks[b])
                sub = s[lists[b]]
                keep = np.flatnonzero(sub > 0)
                keep[np.lexsort((lists[b][keep], -sub[keep]))[:k]]
        w = timed(["scores_walk"], walk, sync, 1, args.reps, args.min_seconds)["scores_walk"]
        rec["lists_1024_x_200"] = {"rows": r["rows"], "scores_walk": dict(w, queries_timed=W, per_query_ms=w["median_ms"] / W,
                                                                            extrapolated_batch_ms=w["median_ms"] / W * B)}
    elif args.section == "sweep":
        lengths = [L for L in (256, 1024, 4096, 16384, 65536, 262144, n // 2) if L <= n // 2]
        cross_col, cross_all = {}, {}
        for L in lengths:
            n_cls = n // L
            dir_id = np.minimum(np.arange(n) // L, n_cls - 1).astype(np.int16)
            eng.set_doc_meta(n, None, dir_id)
            for B in (1, 64, 1024):
                name = f"len_{L}_q_{B}"
                if B * L > args.max_row_scores:
                    rec[name] = "skipped: more (query, row) pairs than --max-row-scores"
                    continue
                cls = np.arange(B) % n_cls
                uniq = np.unique(cls)
                lists = [np.flatnonzero(dir_id == c).astype(np.int64) for c in uniq]
                lo = np.searchsorted(uniq, cls).astype(np.int32)
                r = rec[name] = compare(queries_to_csr(toks[:B]), cls.astype(np.int16), lists, lo, corpus=True)
                if B not in cross_col and r["rows"]["median_ms"] >= r["column"]["median_ms"]:
                    cross_col[B] = L
                if B not in cross_all and r["rows"]["median_ms"] >= r["corpus"]["median_ms"]:
                    cross_all[B] = L
        none = "none up to the longest length measured"
        rec["crossover"] = {f"q_{B}": {"vs_class_column": cross_col.get(B, none), "vs_whole_corpus_scan": cross_all.get(B, none)} for B in (1, 64, 1024)}
    else:
        B, d, kd = 1024, args.dim, 288
        x = synth.dense_corpus_torch(n, d, seed=2, device=dev)
        eng.set_dense(x)
        emb = synth.dense_queries_torch(x, B, seed=1000)
        rng = np.random.default_rng(5)
        dir_id = (np.arange(n) // 200).astype(np.int16)
        eng.set_doc_meta(n, None, dir_id)
        dirs = rng.choice(n // 200, size=B, replace=False)
        lists = [np.arange(200 * c, 200 * c + 200, dtype=np.int64) for c in dirs]
        tabs = RetrievalEngine.lists_to_csr(lists, np.arange(B, dtype=np.int32), B)
        q = queries_to_csr(toks)
        col = dirs.astype(np.int16)

        def fused(arm):
            if arm == "sparse_rows":
                sids, _, sln = eng.bm25_topk_rows_csr(*q, k, *tabs, device_out=True)
            else:
                sids, _, sln = eng.bm25_topk(*q, k, filter_dir=col, device_out=True)
            dids, _, dln = eng.dense_topk_rows_csr(emb, kd, *tabs, device_out=True)
            out = eng.rrf_device(sids, sln, dids, dln, K=60, topk=10)
            eng.sync()
            return out
        rec["dirs_5000_x_200"] = timed(["sparse_column", "sparse_rows"], fused, sync, args.steps, args.reps, args.min_seconds)
    rec["stats"] = eng.stats()
    eng.close()
    with open(args.part, "w") as f:
        json.dump(rec, f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--vocab", type=int, default=262_144)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--k", type=int, default=192)
    ap.add_argument("--sections", default=",".join(SECTIONS))
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--min-seconds", type=float, default=0.3)
    ap.add_argument("--max-row-scores", type=int, default=1 << 26)
    ap.add_argument("--rows-scan", type=int, default=0, choices=(0, 1, 2),
                    help="option bm25_rows_scan for every rows arm: 0 = the row-by-row shapes (default), 1 = by the work rule, 2 = every long list")
    ap.add_argument("--walk-queries", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bm25_rows_timing.json"))
    ap.add_argument("--section", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--part", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.section:
        return section(args)
    rec = {"shape": {"docs": args.docs, "vocab": args.vocab, "variant": "bm25s", "k": args.k, "query_lengths": "the reference's 103 questions"},
           "options": {"bm25_rows_scan": args.rows_scan, "note": "the `rows` arms ran with this value; a default handle has 1 (lists of at least "
                       "bm25_rows_scan_min_rows rows go through the scan where the work rule says so: scripts/rows_scan_timing.py)"},
           "choices": ROWS_CHOICES,
           "method": {"reps": args.reps, "min_seconds": args.min_seconds, "column": "erh_bm25_topk + erh_sync, default options",
                      "rows": "erh_bm25_topk_rows + erh_sync, tables uploaded by every call"}, "sections": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for sec in [s for s in args.sections.split(",") if s]:
            part = os.path.join(tmp, sec + ".json")
            cmd = [sys.executable, os.path.abspath(__file__), "--section", sec, "--part", part, "--docs", str(args.docs), "--vocab", str(args.vocab),
                   "--dim", str(args.dim), "--k", str(args.k), "--steps", str(args.steps), "--reps", str(args.reps),
                   "--min-seconds", str(args.min_seconds), "--max-row-scores", str(args.max_row_scores), "--rows-scan", str(args.rows_scan), "--walk-queries", str(args.walk_queries)]
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
