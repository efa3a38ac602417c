"""Definitions shared by the dense pruning tests (test_gpu_dense_pruning.py) and the parity sweep (test_gpu_dense.py).

The exact dense route answers every query, pruned or not: a query whose candidate list, gather or re-score set overflows, or whose
speculative threshold does not verify, is flagged and answered by the exhaustive path.  Comparing ids and scores therefore cannot see
a defect that only flags more queries.  These helpers say, from fp64 scores alone, what the pruning state of a query MAY be:

  E[q, r]   fp64 score of the fp16 values (a plain fp64 GEMM: its reordering error, ~1e-15, is nine orders below delta)
  delta(q)  d * 2^-23 * |q| * max|x|, DESIGN's bound on |fp32 MFMA score - E|, in fp64 from the fp16 values
  dh        1.01 * delta: absorbs the two 1.0001 factors of the design and the fp32 rounding of the device's margin
  tau       the device's threshold (engine.dense_query_state): an INPUT of the checks, never the expectation

With A the rows a query may see (filter, block):
  L = #{E >= tau + dh}, U = #{E >= tau - dh}         the scan's count lies between them
  T' = tau + 2 delta, nudged up by 1e-6 |.|           the level a speculative threshold is verified at
  n_hi = #{E >= T' + dh}, n_lo = #{E >= T' - dh}     n_hi >= k: verified for sure; n_lo < k: cannot verify
  W = #{E >= kth - 4 dh}                              bounds the re-score set (fp32 >= fp32-kth - 2 delta means exact >= kth - 4 delta)
A query is COMFORTABLE iff U <= 2048 (list and gather cannot overflow), W <= 1024, and its threshold is a guaranteed bound or n_hi >= k:
such a query must not be flagged.
"""
import numpy as np

# (dense_cfg, dense_persist, dense_pp, dense_gemv, dense_speculate, dense_tiled)
SCAN_ARMS = [(0, 1, 3, 0, 1, 0), (0, 1, 3, 0, 1, 1), (0, 1, 3, 0, 0, 0), (0, 0, 0, 0, 1, 0), (0, 0, 0, 0, 0, 0),
             (1, 0, 0, 0, 1, 0), (2, 0, 0, 0, 0, 0), (0, 1, 3, 1, 1, 1)]
SCAN_ARM_IDS = ["pingpong-strict-rowmajor-256x256x32", "pingpong-strict-tiled-256x256x32", "pingpong-strict-rowmajor-guaranteed-bounds",
                "cfg0-256x256x64-per-tile", "cfg0-per-tile-guaranteed-bounds", "cfg1-128x256x32-per-tile",
                "cfg2-256x256x32-per-tile-guaranteed-bounds", "gemv-16x16x32-up-to-64-queries"]
_ARM_OPTIONS = ("dense_cfg", "dense_persist", "dense_pp", "dense_gemv", "dense_speculate", "dense_tiled")
_ARM_DEFAULTS = (0, 1, 3, 1, 1, 0)

FLAG_LIST, FLAG_GATHER, FLAG_RESCORE, FLAG_SPECULATION = 1, 2, 4, 8
LIST_CAP, GATHER_CAP, RESCORE_CAP = 16384, 2048, 1024


def apply_scan_arm(engine, arm):
    for name, value in zip(_ARM_OPTIONS, arm):
        engine.set_option(name, value)


def reset_scan_arm(engine):
    apply_scan_arm(engine, _ARM_DEFAULTS)


def speculative(k: int, n0: int, n: int) -> bool:
    """The host's rule (pipeline_dense.hip) with dense_speculate on: a view of n rows longer than its seed prefix whose seed rank
    (erh_dense_seed_rank) falls below k gets a speculative threshold; every other threshold is a guaranteed bound."""
    from easyrag_amd import _lib
    n0 = min(n0, 32768, n)
    return n > n0 and int(_lib.load().erh_dense_seed_rank(int(k), int(n0), int(n))) < k


def exact_scores(x16: np.ndarray, q16: np.ndarray) -> np.ndarray:
    """E[q, r]: fp64 scores of the fp16 values, [B, N]."""
    return np.atleast_2d(q16).astype(np.float64) @ x16.astype(np.float64).T


def delta_of(x16: np.ndarray, q16: np.ndarray) -> np.ndarray:
    """delta(q) = d * 2^-23 * |q| * max|x| per query, fp64 from the fp16 values."""
    xn = np.sqrt(np.max(np.sum(x16.astype(np.float64) ** 2, axis=1)))
    qn = np.sqrt(np.sum(np.atleast_2d(q16).astype(np.float64) ** 2, axis=1))
    return x16.shape[1] * 2.0 ** -23 * qn * xn


def delta_hat(x16, q16) -> np.ndarray:
    return 1.01 * delta_of(x16, q16)


def kth_score(e_allowed: np.ndarray, k: int) -> float:
    """Exact k-th best score among the allowed rows; -inf with fewer than k of them (the list is then all of them)."""
    if e_allowed.shape[0] < k:
        return -np.inf
    return float(np.partition(e_allowed, e_allowed.shape[0] - k)[e_allowed.shape[0] - k])


def bands(e_allowed: np.ndarray, tau: float, delta: float, k: int) -> dict:
    """The counts of the module docstring for one query: e_allowed = E over A(q), tau from the device, delta = delta(q)."""
    dh = 1.01 * delta
    tau = float(tau)
    kth = kth_score(e_allowed, k)
    lvl = tau + 2.0 * delta
    # the device's own nudge, lvl += |lvl| * 1e-6: UP for either sign ((tau + 2 delta)(1 + 1e-6) for a positive level, (1 - 1e-6) for a
    # negative one), none at a level of zero -- test_gpu_dense_numerics.py exercises negative and zero levels
    lvl = lvl + abs(lvl) * 1e-6 if np.isfinite(lvl) else lvl
    return {"L": int(np.count_nonzero(e_allowed >= tau + dh)), "U": int(np.count_nonzero(e_allowed >= tau - dh)),
            "n_hi": int(np.count_nonzero(e_allowed >= lvl + dh)), "n_lo": int(np.count_nonzero(e_allowed >= lvl - dh)),
            "W": int(np.count_nonzero(e_allowed >= kth - 4.0 * dh)), "kth": kth, "dh": dh, "verifiable": bool(np.isfinite(lvl))}


def comfortable(bd: dict, k: int, speculative: bool) -> bool:
    """(A speculative threshold of -inf -- fewer than k valid prefix rows -- is not verified by the device: nothing is pruned.)"""
    return bd["U"] <= GATHER_CAP and bd["W"] <= RESCORE_CAP and (not speculative or not bd["verifiable"] or bd["n_hi"] >= k)


def check_fast_ranking(ids, scores, e_row: np.ndarray, allowed, k: int, dh: float, what=""):
    """ERH_DENSE_FAST as a ranking.  ids / scores: the returned list of one query (its `len` entries), e_row = E[q, :] over ALL rows,
    allowed = boolean mask of A(q) or None.  Every row clearly above the exact k-th score is listed, no listed row is clearly below it,
    no id twice, every score within dh of the exact score of its row, and the order is right up to 2 dh."""
    ids = np.asarray(ids)
    e_allowed = e_row if allowed is None else e_row[allowed]
    kk = min(k, e_allowed.shape[0])
    assert ids.shape[0] == kk, (what, ids.shape[0], kk)
    assert np.all(ids >= 0) and len(set(ids.tolist())) == kk, f"{what}: an id appears twice"
    if allowed is not None:
        assert np.all(allowed[ids]), f"{what}: a listed row is outside the filter"
    kth = kth_score(e_allowed, kk) if kk else -np.inf
    listed = np.zeros(e_row.shape[0], bool)
    listed[ids] = True
    must = e_row > kth + 2.0 * dh
    if allowed is not None:
        must &= allowed
    assert np.all(listed[must]), f"{what}: {np.count_nonzero(must & ~listed)} rows above kth + 2 dh are missing"
    e_listed = e_row[ids]
    assert np.all(e_listed >= kth - 2.0 * dh), f"{what}: a listed row lies {float(np.max(kth - e_listed)):.3g} below the k-th score"
    err = float(np.max(np.abs(np.asarray(scores) - e_listed))) if kk else 0.0
    assert err <= dh, f"{what}: fp32 score off by {err:.3g} > dh = {dh:.3g}"
    if kk > 1:
        # positions i < j: E[i] >= E[j] - 2 dh  <=>  the running minimum of E before j is >= E[j] - 2 dh
        run_min = np.minimum.accumulate(e_listed)[:-1]
        assert np.all(run_min >= e_listed[1:] - 2.0 * dh), f"{what}: order wrong by more than 2 dh"
