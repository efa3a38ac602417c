"""The handle owns its device memory, and the option table stores what it is told.

Lifetime: every device buffer of the library is a DevBuf that frees itself, and the library counts the bytes its live buffers hold
(erh_debug_live_bytes -> engine.live_device_bytes()); the driver's free-memory figure is no use on a card other processes share.  One
engine goes through every path that allocates, and closing it must give all of it back.  The counter is process-wide and the test
session's shared engine (conftest.py) may be alive, so every figure here is taken relative to the count before the engine under test
exists; in a process of its own that count is 0.

Options: bounds, flags and the measurement names of erh_set_option, and -- through erh_get_option -- that every name is wired to a
field of its own, on its own handle."""
import gc

import numpy as np
import pytest

from easyrag_amd import _lib, synth
from easyrag_amd.engine import RetrievalEngine, live_device_bytes, queries_to_csr
from easyrag_amd.index import BM25S, OKAPI, build_bm25_index

pytestmark = pytest.mark.gpu

N, D, VOCAB, B = 4096, 256, 1024, 8            # the smoke shapes
N_DIRS = 4                                      # dir classes of 1024 consecutive rows


@pytest.fixture(scope="module")
def data():
    x = synth.dense_corpus(N, D, seed=1, dtype=np.float32)
    q = synth.dense_queries(x, B, seed=2)
    flat, lens = synth.token_corpus(N, VOCAB, seed=3, mean_len=24)
    docs = [list(map(int, t)) for t in synth.split_docs(flat, lens)]
    okapi = build_bm25_index(docs, OKAPI)
    queries = synth.token_queries(flat, lens, VOCAB, B, seed=4)
    qi, qt = queries_to_csr([[int(t) for t in qq] for qq in queries])
    return dict(x=x, q=q, flat=flat.astype(np.int32), lens=lens.astype(np.int32), okapi=okapi, qi=qi, qt=qt)


def _baseline() -> int:
    gc.collect()                                # engines other tests dropped without close() go now, not in the middle of a measurement
    return live_device_bytes()


def _exercise(eng, data):
    """Every allocating path of the library, once."""
    eng.set_option("dense_dir_block_min_rows", 512)                       # so that the four dir blocks get copies of their own
    eng.set_dense(data["x"])                                              # fp32 host rows: the slab staging
    eng.set_doc_meta(N, np.arange(N, dtype=np.int32), (np.arange(N) * N_DIRS // N).astype(np.int16))
    q = data["q"]
    eng.dense_topk(q, 10)                                                 # host output
    filt = (np.arange(B) % N_DIRS).astype(np.int16)
    eng.dense_topk(q, 10, filter_dir=filt)                                # builds the block copies; this small, it still scans with the filter column
    eng.set_option("dense_dir_blocks", 2)                                 # ... and routed by block: the group tables and lists
    eng.dense_topk(q, 10, filter_dir=filt)
    assert eng.stats()["dense_block_groups"] > 0
    eng.dense_topk_sets(q, 10, [[0, 1]] * B)
    eng.dense_topk_rows(q, 10, [np.arange(100), np.arange(3000)], list_of=np.arange(B) % 2)   # the short and the long shape
    st = eng.stats()
    assert st["dense_rows_short_launches"] > 0 and st["dense_rows_long_launches"] > 0
    eng.build_bm25(data["flat"], data["lens"], VOCAB, BM25S, slot=0, fetch=False)              # index built on the device
    eng.set_bm25(data["okapi"], payload_on_device=True, slot=1)                                # Okapi through the tf upload
    qi, qt = data["qi"], data["qt"]
    ids_a, sc_a, len_a = eng.bm25_topk(qi, qt, 20, slot=0)
    eng.bm25_scores(data["okapi"].tokens_to_ids([int(t) for t in qt[qi[0]:qi[1]]]), slot=1)     # (the host index numbers its own vocabulary)
    eng.bm25_scores(qt[qi[0]:qi[1]], slot=0)
    eng.hybrid_topk(q, qi, qt, k_dense=32, k_sparse=20, K=60, topk=10, slot=0)
    ids_b, sc_b, len_b = eng.dense_topk(q, 20)
    eng.rrf(ids_a, len_a, ids_b, len_b, K=60, topk=10)
    eng.fusion(ids_a, sc_a, len_a, ids_b, sc_b, len_b, topk=10)
    eng.get_dense_rows(0, 16)
    eng.free_bm25_slot(1)                                                 # erh_bm25_release


def test_close_frees_every_device_byte(data):
    base = _baseline()
    eng = RetrievalEngine(0)
    try:
        _exercise(eng, data)
        assert live_device_bytes() - base > 0
    finally:
        eng.close()
    assert live_device_bytes() - base == 0


def test_create_use_close_repeated(data):
    base = _baseline()
    for rep in range(3):
        eng = RetrievalEngine(0)
        try:
            _exercise(eng, data)
        finally:
            eng.close()
        assert live_device_bytes() - base == 0, rep


def test_index_build_temporaries_do_not_accumulate(data):
    base = _baseline()
    eng = RetrievalEngine(0)
    try:
        eng.build_bm25(data["flat"], data["lens"], VOCAB, BM25S, fetch=False)
        first = live_device_bytes()
        eng.build_bm25(data["flat"], data["lens"], VOCAB, BM25S, fetch=False)
        assert live_device_bytes() == first
        assert first - base > 0
    finally:
        eng.close()
    assert live_device_bytes() - base == 0


def test_rejected_index_build_leaks_nothing(data):
    base = _baseline()
    bad = data["flat"].copy()
    bad[5] = VOCAB                                                        # refused by the key kernel's range check: nothing is indexed with it
    eng = RetrievalEngine(0)
    try:
        with pytest.raises(_lib.ErhError) as ei:
            eng.build_bm25(bad, data["lens"], VOCAB, BM25S, fetch=False)
        assert ei.value.status == _lib.ERH_ERR_INVALID
    finally:
        eng.close()
    assert live_device_bytes() - base == 0


# ---- options ---------------------------------------------------------------------------------------------------------------------
# name: (lo, hi); hi None = no upper bound; n_cus: the device's CU count, filled in by the test
RANGES = {
    "dense_n0": (1, None), "dense_n1": (0, None), "dense_cfg": (0, 2), "dense_pp": (0, 4), "dense_selfseed": (0, 2),
    "n_cus": (0, "cus"), "bm25_long_tokens": (0, 4096), "bm25_long_segs": (1, 16), "dense_rows_ws_mb": (0, 65536),
    "dense_route_ridge": (1, 4096), "dense_dir_blocks": (0, 2), "dense_dir_block_min_rows": (1, None), "dense_var": (0, 3),
    "dense_rot": (-1, 4096), "dense_gemv_pipe": (-1, 1), "dense_gemv_nt": (-1, 1), "dense_fin_wgs": (2, 4),
    "dense_gemv_wgs": (1, 5), "comm_timeout_s": (1, 86400), "bm25_segs": (0, 64), "bm25_crossing": (0, 2),
    "hybrid_overlap": (-1, 2), "bm25_fine_max_mb": (0, None),
}
FLAGS = ["dense_readahead", "dense_shuffle", "dense_n1_auto", "dense_n0_auto", "dense_sync",
         "bm25_split_finish", "bm25_mixed", "dense_group_sample", "dense_group_launch", "bm25_dir_range",
         "dense_fin_split", "dense_tile384", "dense_tiled", "dense_speculate", "dense_gemv",
         "dense_scan_nt", "dense_small_single_stage", "dense_persist",
         "bm25_lpt", "bm25_ascan", "bm25_post16", "bm25_wscan"]
MEASURE = ["dense_ablate", "bm25_ablate", "debug_counters"]
# a valid value that is not the default, for every option that holds a number
NON_DEFAULT = {
    "dense_n0": 12345, "dense_n1": 54321, "dense_cfg": 2, "dense_pp": 1, "dense_selfseed": 2, "n_cus": 7, "bm25_long_tokens": 100,
    "bm25_long_segs": 3, "dense_rows_ws_mb": 17, "dense_route_ridge": 99, "dense_dir_blocks": 2, "dense_dir_block_min_rows": 777,
    "dense_var": 3, "dense_rot": 5, "dense_gemv_pipe": 1, "dense_gemv_nt": 0, "dense_fin_wgs": 2, "dense_gemv_wgs": 5,
    "comm_timeout_s": 33, "bm25_segs": 9, "bm25_crossing": 2, "hybrid_overlap": 2, "bm25_fine_max_mb": 11,
    "dense_gemv_kb": 16, "bm25_small": 1, "dense_tile384_max_mb": 123,
}


def _status(eng, name, value) -> int:
    return eng._lib.erh_set_option(eng._h, name.encode(), int(value))


def _device_cus() -> int:
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def check_option_acceptance(eng, cus):
    """What erh_set_option takes and what it refuses (status codes only)."""
    for name, (lo, hi) in RANGES.items():
        hi = cus if hi == "cus" else hi
        assert _status(eng, name, lo) == _lib.ERH_OK, name
        assert _status(eng, name, lo - 1) == _lib.ERH_ERR_INVALID, name
        if hi is None:
            assert _status(eng, name, 1 << 40) == _lib.ERH_OK, name
        else:
            assert _status(eng, name, hi) == _lib.ERH_OK, name
            assert _status(eng, name, hi + 1) == _lib.ERH_ERR_INVALID, name
    assert _status(eng, "dense_gemv_kb", 16) == _lib.ERH_OK and _status(eng, "dense_gemv_kb", 32) == _lib.ERH_OK
    assert _status(eng, "dense_gemv_kb", 24) == _lib.ERH_ERR_INVALID
    assert _status(eng, "bm25_small", -5) == _lib.ERH_OK and _status(eng, "bm25_small", 9) == _lib.ERH_OK
    for name in FLAGS:
        for v in (0, 1, 7, -3):
            assert _status(eng, name, v) == _lib.ERH_OK, (name, v)
    for name in MEASURE:                                                  # the product build
        assert _status(eng, name, 0) == _lib.ERH_OK, name
        assert _status(eng, name, 1) == _lib.ERH_ERR_UNSUPPORTED, name
    assert _status(eng, "no_such_option", 0) == _lib.ERH_ERR_INVALID


def test_option_bounds_and_readback():
    cus = _device_cus()
    eng = RetrievalEngine(0)
    other = RetrievalEngine(0)
    try:
        check_option_acceptance(eng, cus)
        # what was stored
        for v, want in ((-5, 0), (9, 2)):
            eng.set_option("bm25_small", v)
            assert eng.get_option("bm25_small") == want
        for name in FLAGS:
            for v, want in ((7, 1), (0, 0), (-3, 1)):
                eng.set_option(name, v)
                assert eng.get_option(name) == want, (name, v)
        for name in MEASURE:
            assert eng.get_option(name) == 0
        eng.set_option("n_cus", 0)
        assert eng.get_option("n_cus") == cus                             # 0 = all of the device
        with pytest.raises(_lib.ErhError) as ei:
            eng.get_option("no_such_option")
        assert ei.value.status == _lib.ERH_ERR_INVALID
        # every name has a field of its own: one option at a time moves to a value it did not hold, and nothing else moves with it
        names = list(NON_DEFAULT) + FLAGS
        assert set(RANGES) <= set(NON_DEFAULT)
        fresh = RetrievalEngine(0)
        try:
            state = {n: fresh.get_option(n) for n in names}
            for n in names:
                v = NON_DEFAULT[n] if n in NON_DEFAULT else 1 - state[n]
                assert v != state[n], n
                fresh.set_option(n, v)
                state[n] = v
                assert {m: fresh.get_option(m) for m in names} == state, n
            # ... so that in the end every option reads back what it was set to
            assert {n: fresh.get_option(n) for n in NON_DEFAULT} == NON_DEFAULT
        finally:
            fresh.close()
        # ... on its own handle
        eng.set_option("dense_fin_wgs", 2)
        assert eng.get_option("dense_fin_wgs") == 2 and other.get_option("dense_fin_wgs") == 4
    finally:
        eng.close()
        other.close()
