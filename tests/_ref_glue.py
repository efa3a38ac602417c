"""Loader of the reference-glue fixture (tests/golden/ref_glue.json + its two .npz files, written by
tests/golden/make_ref_glue_fixture.py from the reference's own code).  Shared by test_ref_glue_fixture.py (CPU) and
test_gpu_ref_glue.py (GPU); reads nothing outside tests/golden/."""
from __future__ import annotations

import functools
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILES = ("ref_glue.json", "ref_glue_fusion.npz", "ref_glue_corpus.npz")


@functools.lru_cache(maxsize=1)
def load():
    with open(os.path.join(GOLDEN, "ref_glue.json"), encoding="utf-8") as f:
        data = json.load(f)
    with np.load(os.path.join(GOLDEN, "ref_glue_fusion.npz")) as z:
        fusion = {k: z[k] for k in z.files}
    with np.load(os.path.join(GOLDEN, "ref_glue_corpus.npz")) as z:
        corpus = {k: z[k] for k in z.files}
    return data, fusion, corpus


def floats(hexes) -> np.ndarray:
    return np.asarray([float.fromhex(h) for h in hexes], np.float64)


def filter_scores(case) -> np.ndarray:
    return floats(case["scores"]).astype(case["dtype"])


def fuse_cases():
    """Every fusion case with its arrays resolved: (name, cid int64[n], score f64[n], lens, modes) where
    modes[m] = (pos int64[n_distinct], score f64[n_distinct], {topk: length})."""
    data, arrs, _ = load()
    out = []
    for c in data["fuse"]:
        name = c["name"]
        if c["cid"] == "npz":
            cid, sc = arrs[f"{name}/cid"].astype(np.int64), arrs[f"{name}/score"]
        else:
            cid, sc = np.asarray(c["cid"], np.int64), floats(c["score"])
        modes = {}
        for m in [k for k in c if k == "fusion" or k.startswith("rrf_K")]:
            rec = c[m]
            pos = arrs[f"{name}/{m}/pos"].astype(np.int64) if rec["pos"] == "npz" else np.asarray(rec["pos"], np.int64)
            if rec["score"] == "input":
                osc = sc[pos] if len(pos) else np.zeros(0)
            elif rec["score"] == "npz":
                osc = arrs[f"{name}/{m}/score"]
            else:
                osc = floats(rec["score"])
            modes[m] = (pos, osc, {int(t): n for t, n in rec["topk_len"].items()})
        out.append((name, cid, sc, list(c["lens"]), modes))
    return out


def rrf_K(mode: str):
    return None if mode == "fusion" else int(mode[len("rrf_K"):])


def bits(a) -> np.ndarray:
    return np.asarray(a, np.float64).view(np.uint64)


def composition_texts():
    """(doc texts, doc metadata, query texts, query dir filters or None) of the composition corpus."""
    data, _, z = load()
    comp = data["composition"]
    lens = z["doc_tok_len"].astype(np.int64)
    flat = z["doc_tok_flat"].astype(np.int64)
    starts = np.concatenate([[0], np.cumsum(lens)])
    texts = [" ".join(f"t{t}" for t in flat[starts[i]:starts[i + 1]]) for i in range(len(lens))]
    dirs = comp["dirs"]
    meta = [{"dir": dirs[int(d)], "know_path": f"kp{int(k) // 4} sec{int(k) % 4}"}
            for d, k in zip(z["doc_dir"], z["doc_kp"])]
    queries = [" ".join(t) for t in comp["query_tokens"]]
    qfilt = [None if int(d) < 0 else {"dir": dirs[int(d)]} for d in z["query_dir"]]
    return texts, meta, queries, qfilt
