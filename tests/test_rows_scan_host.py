"""The host step of the rows entries' scan route (DESIGN K11), without a device: the cells of a call -- rows with the same membership
signature over the routed lists -- become each query's class set.  The signatures are computed here the way the device computes them (bit l
of a row's word = the row is in routed list l; a cell per distinct non-zero word), the class sets come from the library
(erh_debug_rows_class_sets), and the union of a query's cells must be its list, cell for cell disjoint.  Plus: the new option and stat names
are in the header and the Python tables."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from easyrag_amd import _lib

ROOT = Path(__file__).resolve().parents[1]
OPTIONS = ("dense_rows_scan", "bm25_rows_scan", "dense_rows_scan_min_rows", "bm25_rows_scan_min_rows", "dense_rows_scan_gain",
           "dense_rows_scan_small_cell", "bm25_rows_scan_gain", "bm25_rows_scan_floor")
STATS = ("dense_rows_scan_calls", "dense_rows_scan_subqueries", "bm25_rows_scan_calls", "bm25_rows_scan_subqueries",
         "dense_block_builds")


def _cells(n, lists):
    """Distinct non-zero signatures of n rows over `lists`, in a shuffled order (the device's numbering is not deterministic), and the rows
    of each."""
    sig = np.zeros(n, np.uint64)
    for l, rows in enumerate(lists):
        sig[np.asarray(rows, np.int64)] |= np.uint64(1) << np.uint64(l)
    vals = np.unique(sig[sig != 0])
    vals = vals[np.random.default_rng(len(lists)).permutation(len(vals))]
    return vals, [np.flatnonzero(sig == v) for v in vals]


def _class_sets(cell_sig, n_routed, bit_of, cap=1 << 16):
    lib = _lib.load()
    cell_sig = np.ascontiguousarray(cell_sig, np.uint64)
    bit_of = np.ascontiguousarray(bit_of, np.int32)
    B = bit_of.shape[0]
    ptr = np.full(B + 1, -7, np.int32)
    cls = np.full(cap, -7, np.int16)
    rc = lib.erh_debug_rows_class_sets(len(cell_sig), cell_sig.ctypes.data, n_routed, B, bit_of.ctypes.data, ptr.ctypes.data, cls.ctypes.data, cap)
    return rc, ptr, cls


CASES = {
    "one list": (50, [np.arange(3, 40)], [0, 0, -1, 0]),
    "two disjoint lists": (60, [np.arange(0, 25), np.arange(30, 60)], [0, 1, 1, -1, 0]),
    "two overlapping lists": (60, [np.arange(0, 40), np.arange(20, 60)], [1, 0, 1]),
    "nested lists": (80, [np.arange(0, 80, 2), np.arange(0, 80, 4), np.arange(0, 80, 8)], [2, 1, 0, 0]),
    "a list of all rows": (33, [np.arange(33), np.arange(5, 9)], [0, 1]),
    "64 lists": (700, [np.arange(l, 700, l + 1) for l in range(64)], list(range(64)) + [-1, 5]),
}


@pytest.mark.parametrize("name", list(CASES))
def test_class_sets_of_hand_made_lists(name):
    n, lists, bit_of = CASES[name]
    sig, rows_of = _cells(n, lists)
    want_cells = {"one list": 1, "two disjoint lists": 2, "two overlapping lists": 3, "nested lists": 3, "a list of all rows": 2}
    if name in want_cells:
        assert len(sig) == want_cells[name]
    rc, ptr, cls = _class_sets(sig, len(lists), bit_of)
    assert rc == _lib.ERH_OK
    assert ptr[0] == 0 and np.all(np.diff(ptr) >= 0)
    for b, l in enumerate(bit_of):
        mine = cls[ptr[b]:ptr[b + 1]]
        if l < 0:
            assert len(mine) == 0, (name, b)
            continue
        assert len(mine) > 0 and np.all(np.diff(mine) > 0) and mine.min() >= 0 and mine.max() < len(sig), (name, b)
        # exactly the cells whose signature has the list's bit ...
        assert set(int(c) for c in mine) == {c for c in range(len(sig)) if (int(sig[c]) >> l) & 1}, (name, b)
        # ... and their rows are the list, every row once
        got = np.sort(np.concatenate([rows_of[c] for c in mine]))
        assert np.array_equal(got, np.asarray(lists[l], np.int64)), (name, b)
    assert np.all(cls[ptr[-1]:] == -7)                                      # nothing written behind the sets


def test_fall_backs_and_bad_arguments():
    # 65 routed lists: more than a signature word has bits -> the call keeps the row-by-row shapes
    sig = np.array([1, 2, 3], np.uint64)
    assert _class_sets(sig, 65, [0, 1])[0] == _lib.ERH_ERR_UNSUPPORTED
    assert _class_sets(sig, 64, [0, 1])[0] == _lib.ERH_OK
    # more cells than an int16 column can number (32767 is "matches nothing")
    many = np.arange(1, 32768, dtype=np.uint64)
    assert _class_sets(many, 15, [0], cap=1 << 20)[0] == _lib.ERH_ERR_UNSUPPORTED
    rc, ptr, cls = _class_sets(many[:32766], 15, [0, 14], cap=1 << 20)
    assert rc == _lib.ERH_OK and ptr[1] == 16383 and ptr[2] - ptr[1] == 16383     # odd signatures; those with bit 14
    # the caller's array is too small: refused, not overrun
    rc, ptr, cls = _class_sets(sig, 2, [0, 1, 1], cap=3)
    assert rc == _lib.ERH_ERR_NOMEM and np.all(cls == -7)
    assert _class_sets(sig, 2, [0, 1, 1], cap=6)[0] == _lib.ERH_OK
    # no query on the route, no cells
    rc, ptr, cls = _class_sets(np.zeros(0, np.uint64), 0, [-1, -1])
    assert rc == _lib.ERH_OK and list(ptr) == [0, 0, 0]
    lib = _lib.load()
    assert lib.erh_debug_rows_class_sets(1, None, 1, 0, None, None, None, 0) == _lib.ERH_ERR_INVALID


def test_new_names_are_in_the_header_and_the_python_tables():
    from easyrag_amd.engine import RetrievalEngine
    header = (ROOT / "include" / "easyrag_hip.h").read_text()
    for name in OPTIONS + STATS:
        assert re.search(r"\b%s\b" % name, header), name
    for name in STATS:
        assert name in RetrievalEngine.STAT_NAMES, name
    assert "erh_debug_rows_class_sets" in _lib.SIGNATURES
    api = (ROOT / "easyrag_amd" / "csrc" / "api.hip").read_text()
    for name in OPTIONS + STATS:
        assert '"%s"' % name in api, name
