"""GPU parity of the 16x16x32 body of the 384 x 256 dense scan (dense_scan_pp5_kernel<1>, option dense_mfma16): every case runs with
dense_mfma16 = 1 and = 0; both arms must be bit-equal to each other (ids, fp64 score bits, lengths) and to the oracle, and
erh_get_stat proves which body ran (dense_scan_mf16_launches).

What can go wrong in this body and nowhere else: the fragment addresses (row lane & 15, slot lane >> 4), the rolling ring of
chunk-side fragments (a block meeting the wrong accumulator), the accumulator -> (row, query) formula of the epilogue and the
threshold slot a lane reads.  The shapes are the smallest that reach the kernel (Bpad >= 512, d >= 256, d % 64 == 0, N >= 768,
scan start on a multiple of 384; see tests/test_gpu_dense_tile384.py).
"""
import numpy as np
import pytest

from easyrag_amd import synth
from oracle import dense_exact_topk, to_f16_unit

pytestmark = pytest.mark.gpu


def _bits(a):
    a = np.asarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _both_bodies(engine, call):
    """`call()` with dense_mfma16 = 1, then = 0 (the option is left as it was found); returns the first arm's (result, diag, stats)."""
    was = engine.get_option("dense_mfma16")
    out = []
    try:
        for mf in (1, 0):
            engine.set_option("dense_mfma16", mf)
            assert engine.get_option("dense_mfma16") == mf
            engine.reset_stats()
            res = call()
            diag = engine.dense_diag()
            st = engine.stats()
            assert st["dense_scan_pp5_launches"] >= 1, f"the 384 x 256 kernel did not run: {st}"
            if mf:
                assert st["dense_scan_mf16_launches"] >= 1, st
                assert st["dense_scan_mf16_launches"] == st["dense_scan_pp5_launches"], st
            else:
                assert st["dense_scan_mf16_launches"] == 0, st
            out.append((res, diag, st))
    finally:
        engine.set_option("dense_mfma16", was)
    (a, da, _), (b, db, _) = out
    for x, y in zip(a, b):
        assert np.array_equal(_bits(x), _bits(y)), "the 16x16x32 and the 32x32x16 bodies disagree"
    assert da["exhaustive"] == db["exhaustive"] and da["uncertified"] == db["uncertified"]
    return out[0]


def _check(x, q16, ids, sc, ln, k, which, mask_of=None):
    for i in which:
        mask = None if mask_of is None else mask_of(i)
        oid, osc = dense_exact_topk(x, q16[i], k, mask)
        assert ln[i] == len(oid), f"query {i}: length {ln[i]} != {len(oid)}"
        assert np.array_equal(ids[i, :ln[i]], oid), f"query {i}: ids differ"
        assert np.array_equal(sc[i, :ln[i]].view(np.uint64), osc.view(np.uint64)), f"query {i}: fp64 scores differ"
        assert np.all(ids[i, ln[i]:] == -1)


def _options(engine, pairs):
    for name, v in pairs:
        engine.set_option(name, v)


def test_option_is_a_flag_and_reads_back(engine):
    was = engine.get_option("dense_mfma16")
    try:
        for v, want in ((7, 1), (0, 0), (-3, 1), (1, 1)):
            engine.set_option("dense_mfma16", v)
            assert engine.get_option("dense_mfma16") == want
    finally:
        engine.set_option("dense_mfma16", was)
    assert "dense_scan_mf16_launches" in engine.stats()


@pytest.mark.parametrize("d", [256, 320])              # 8 stages (the minimum) / 10: an odd number of stage pairs
@pytest.mark.parametrize("n", [769, 2 * 384 + 165])
def test_mfma16_every_accumulator_position_returns_its_own_row(engine, n, d):
    """520 queries (three query tiles, the last mostly padding); the seed prefix is one 384-row tile, so the 384 x 256 kernel scans rows
    384 .. N - 1 in the caller's order (row placement off).  Query i's copy is planted at row 384 + (7 i mod 384) of the first
    scanned tile (7 is a unit mod 384: distinct rows), queries 384 .. 519 repeat queries 0 .. 135 -- the same rows under query
    columns 128 further on -- or, where the second tile has the rows, get copies of their own there.  A wrong row or query
    formula in the fragment addresses or in the epilogue returns a wrong id, not a tie."""
    b, k = 520, 10
    rng = np.random.default_rng(1000 + n + d)
    x = to_f16_unit(rng.standard_normal((n, d)))
    q16 = to_f16_unit(rng.standard_normal((b, d)))
    pos = np.empty(b, np.int64)
    for i in range(384):
        pos[i] = 384 + (7 * i) % 384
    tail_rows = n - 768
    for i in range(384, b):
        if tail_rows >= b - 384:
            pos[i] = 768 + (7 * (i - 384)) % tail_rows       # (7 is a unit mod 165)
        else:
            q16[i] = q16[i - 384]
            pos[i] = pos[i - 384]
    assert len(set(pos[:384])) == 384 and (tail_rows < b - 384 or len(set(pos)) == b)
    x[pos] = q16
    # the positions cover every part of the layout: 2 wave groups x 12 row blocks, the four 4-row lane groups, the four rows of a
    # lane, the four wave columns x four query blocks x 16 lanes
    p, qc = pos[:384] - 384, np.arange(384) % 256
    assert {(int(a) // 192, int(a) % 192 // 16) for a in p} == {(g, m) for g in range(2) for m in range(12)}
    assert {int(a) % 16 // 4 for a in p} == set(range(4)) and {int(a) % 4 for a in p} == set(range(4))
    assert {(int(c) // 64, int(c) % 64 // 16, int(c) % 16) for c in qc} == {(w, t, l) for w in range(4) for t in range(4) for l in range(16)}
    _options(engine, (("dense_n0", 384), ("dense_gemv", 0), ("dense_shuffle", 0)))
    try:
        engine.set_dense(x)
        (ids, sc, ln), diag, st = _both_bodies(engine, lambda: engine.dense_topk(q16, k))
    finally:
        _options(engine, (("dense_n0", 32768), ("dense_gemv", 1), ("dense_shuffle", 1)))
    assert diag["uncertified"] == 0 and np.all(ln == k)
    assert np.array_equal(ids[:, 0], pos), np.flatnonzero(ids[:, 0] != pos)[:20]
    _check(x, q16, ids, sc, ln, k, range(b))


def _tie_block_case():
    """The shape of test_tile384_tie_block_floods_the_record_buffers: 600 identical queries, 600 copies of them in consecutive tiles."""
    rng = np.random.default_rng(21)
    n, d, b, k = 70000, 256, 600, 100
    x = to_f16_unit(rng.standard_normal((n, d)))
    hot = to_f16_unit(rng.standard_normal((1, d)))[0]
    x[40010:40610] = hot                                          # (straddles 384-row tile boundaries)
    return x, hot, np.repeat(hot[None, :], b, axis=0), k


def test_mfma16_tie_block_floods_the_record_buffers(engine):
    """Every (chunk, query) pair of the tie block's tiles survives the threshold: 12288 hits per wave and tile against the 190-record
    buffer, so every wave walks the overflow loop (`over_` / `shift_`) dozens of times on the 16 x 16 record layout."""
    x, hot, q16, k = _tie_block_case()
    b = q16.shape[0]
    _options(engine, (("dense_shuffle", 0), ("dense_gemv", 0)))
    try:
        engine.set_dense(x)
        (ids, sc, ln), diag, st = _both_bodies(engine, lambda: engine.dense_topk(q16, k))
    finally:
        _options(engine, (("dense_shuffle", 1), ("dense_gemv", 1)))
    assert st["dense_sample_passes"] == 1 and diag["uncertified"] == 0 and diag["exhaustive"] == 0
    oid, osc = dense_exact_topk(x, hot, k)
    assert np.array_equal(oid, np.arange(40010, 40110))
    for i in (0, 1, 15, 16, 63, 64, 255, 256, 511, 512, b - 1):
        assert ln[i] == k and np.array_equal(ids[i], oid) and np.array_equal(sc[i].view(np.uint64), osc.view(np.uint64)), i


def test_mfma16_duplicates_and_filter_column(engine):
    """2 % exact duplicate rows and a dir filter on every query: the flush's dir_id[chunk] test on rows decoded from the 16 x 16 records
    (the filter COLUMN, block copies off); staged path with a seed prefix of 4 x 384 rows."""
    n, d, b, k = 5000, 256, 520, 288
    rng = np.random.default_rng(5)
    x = to_f16_unit(rng.standard_normal((n, d)))
    dup = rng.choice(n, size=n // 50, replace=False)
    x[dup] = x[rng.choice(np.setdiff1d(np.arange(n), dup), size=dup.size, replace=False)]
    q16 = to_f16_unit(x[rng.integers(0, n, size=b)].astype(np.float32) + 0.05 * rng.standard_normal((b, d)))
    dir_id = (np.arange(n) % 3).astype(np.int16)
    filt = rng.integers(0, 3, size=b).astype(np.int16)
    _options(engine, (("dense_n0", 1536), ("dense_gemv", 0), ("dense_dir_blocks", 0)))
    try:
        engine.set_dense(x)
        engine.set_doc_meta(n, None, dir_id)
        (ids, sc, ln), diag, st = _both_bodies(engine, lambda: engine.dense_topk(q16, k, filter_dir=filt))
    finally:
        _options(engine, (("dense_dir_blocks", 1), ("dense_n0", 32768), ("dense_gemv", 1)))
        engine.set_doc_meta(n, None, None)
    assert st["dense_sample_passes"] == 0 and diag["uncertified"] == 0
    _check(x, q16, ids, sc, ln, k, list(range(0, b, 13)) + [255, 256, 511, 512, b - 1], mask_of=lambda i: dir_id == filt[i])


def test_mfma16_partial_last_tile(engine):
    """N = 4 x 384 + 1: the last scanned tile holds one row and 383 rows of zero padding; k = N - 1 clipped to the maximum (768) admits
    almost everything, and no row >= N may come back."""
    n, d, b = 4 * 384 + 1, 256, 512
    k = min(n - 1, 768)
    x = synth.dense_corpus(n, d, seed=n)
    q16 = to_f16_unit(synth.dense_queries(x, b, seed=k))
    _options(engine, (("dense_n0", 384), ("dense_gemv", 0)))
    try:
        engine.set_dense(x)
        (ids, sc, ln), diag, st = _both_bodies(engine, lambda: engine.dense_topk(q16, k))
    finally:
        _options(engine, (("dense_n0", 32768), ("dense_gemv", 1)))
    assert np.all(ln == k) and diag["uncertified"] == 0
    assert ids.min() >= 0 and ids.max() < n
    _check(x, q16, ids, sc, ln, k, [0, 1, 15, 16, 255, 256, 300, b - 1])


def test_mfma16_guaranteed_bounds_and_refinement_stages(engine):
    """dense_speculate = 0 on 128 CUs: guaranteed thresholds refined between append launches -- several launches of the 16x16x32 body per
    call, each with c0 > 0 and clamped at its own c1."""
    n, d, b, k = 40000, 256, 520, 50
    x = synth.dense_corpus(n, d, seed=77)
    q16 = to_f16_unit(synth.dense_queries(x, b, seed=78))
    _options(engine, (("dense_speculate", 0), ("dense_n0", 768), ("dense_n1", 3072), ("dense_n1_auto", 0), ("dense_gemv", 0), ("n_cus", 128)))
    try:
        engine.set_dense(x)
        (ids, sc, ln), diag, st = _both_bodies(engine, lambda: engine.dense_topk(q16, k))
    finally:
        _options(engine, (("dense_speculate", 1), ("dense_n0", 32768), ("dense_n1", 131072), ("dense_n1_auto", 1), ("dense_gemv", 1), ("n_cus", 0)))
    assert st["dense_scan_mf16_launches"] >= 2 and st["dense_scan_pp3_launches"] == 0, st
    assert diag["uncertified"] == 0 and diag["exhaustive"] == 0
    _check(x, q16, ids, sc, ln, k, [0, 1, 2, 15, 16, 255, 256, 511, 512, b - 1])
