"""The true-peak meter's committed table (csrc/tl_truepeak_taps.inc): the properties the header states -- every row sums to 32768, row 3 is
row 1 reversed, row 2 is symmetric, a whole row times full scale stays inside 32 bits -- tools/gen_truepeak_taps.py reproduces it, the
library hands out the same numbers, and TLB_TRUEPEAK_CEILING_DEFAULT is -1 dBTP."""
import importlib.util
import re
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
INC = ROOT / "odr-audioenc_amd" / "csrc" / "tl_truepeak_taps.inc"
HEADER = ROOT / "include" / "toolame_batch.h"


def _gen():
    spec = importlib.util.spec_from_file_location("gen_truepeak_taps", ROOT / "tools" / "gen_truepeak_taps.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _committed():
    """the table of the .inc as written -> int64 [3][T]"""
    m = re.search(r"static const int16_t tl_truepeak_taps\[3\]\[(\d+)\] = \{(.*?)\};", INC.read_text(), flags=re.S)
    body = re.sub(r"//[^\n]*", "", m.group(2))
    return np.array([int(v) for v in re.findall(r"-?\d+", body)], dtype=np.int64).reshape(3, int(m.group(1)))


def test_the_table_has_the_properties_the_header_states():
    H = _committed()
    assert H.shape == (3, 12)
    assert (H.sum(axis=1) == 32768).all()
    assert (H[2] == H[0][::-1]).all() and (H[1] == H[1][::-1]).all()
    assert np.abs(H).max() < 32768                                   # an int16 holds every tap
    worst = int(np.abs(H).sum(axis=1).max())
    print("max_p sum_t |H[p][t]| = %d" % worst)
    assert worst * 32768 < 2 ** 31                                   # a whole row is summed in 32 bits
    assert worst == 57760                                            # the figure the header prints


def test_generator_reproduces_the_committed_table():
    assert _gen().text() == INC.read_text()


def test_the_library_returns_the_table():
    import odr_audioenc_amd as M
    if not M.LIB_PATH.exists():
        M.build()
    got = M.truepeak_taps()
    assert got.dtype == np.int16 and got.shape == (3, M.TRUEPEAK_TAPS) and (got == _committed()).all()
    assert M.load_library().tlb_truepeak_taps(None) == 18
    assert re.search(r"#define\s+TLB_TRUEPEAK_TAPS\s+12\b", HEADER.read_text())


def test_the_default_ceiling_is_minus_1_dbtp():
    import odr_audioenc_amd as M
    want = int(round(2.0 ** 30 * 10.0 ** (-1.0 / 20.0)))
    m = re.search(r"#define\s+TLB_TRUEPEAK_CEILING_DEFAULT\s+(\d+)u\b", HEADER.read_text())
    assert m and int(m.group(1)) == want == M.TRUEPEAK_CEILING_DEFAULT
