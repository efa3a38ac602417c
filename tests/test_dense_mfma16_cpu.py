"""Host-side checks of the dense_mfma16 option and its stat (no device needed): the names are in the public header's option and stat
lists, in the one option table of api.hip as a flag, and in the Python stat table.  That the option is accepted, stored as 0 / 1 and
read back needs a handle, i.e. a device: tests/test_gpu_dense_mfma16.py::test_option_is_a_flag_and_reads_back."""
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
OPTION, STAT = "dense_mfma16", "dense_scan_mf16_launches"


def test_option_and_stat_are_in_the_header_the_option_table_and_the_python_tables():
    from easyrag_amd.engine import RetrievalEngine
    header = (ROOT / "include" / "easyrag_hip.h").read_text()
    m = re.search(r"^ \*   %s \((-?\d+)\)" % OPTION, header, flags=re.M)
    assert m, "the option list of the header has no entry for " + OPTION
    assert re.search(r"^ \*   %s\b" % STAT, header, flags=re.M)
    api = (ROOT / "easyrag_amd" / "csrc" / "api.hip").read_text()
    assert re.search(r'opt_flag\("%s", &H::opt_dense_mfma16\)' % OPTION, api)          # a flag: any integer is accepted, stored as 0 / 1
    assert '{"%s", T.dense_scan_mf16}' % STAT in api
    assert STAT in RetrievalEngine.STAT_NAMES
    # the default the header documents is the one the handle starts with
    handle = (ROOT / "easyrag_amd" / "csrc" / "handle.h").read_text()
    d = re.search(r"int opt_dense_mfma16 = (\d+);", handle)
    assert d and d.group(1) == m.group(1)


def test_both_bodies_are_instantiated_and_selected_by_the_option():
    scan = (ROOT / "easyrag_amd" / "csrc" / "dense_scan.hip").read_text()
    assert "dense_scan_pp5_kernel<0>" in scan and "dense_scan_pp5_kernel<1>" in scan
    pipe = (ROOT / "easyrag_amd" / "csrc" / "pipeline_dense.hip").read_text()
    assert "h->opt_dense_mfma16 != 0, st)" in pipe and "dense_scan_mf16 +=" in pipe
