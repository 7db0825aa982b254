"""The loudness meter's committed table (csrc/tl_loudness_tables.inc): tools/gen_loudness_tables.py reproduces it, its 48 kHz row is the
pair of filters ITU-R BS.1770-4 prints, the gating scale is ordered, and the library hands out the same doubles."""
import importlib.util
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
INC = ROOT / "odr-audioenc_amd" / "csrc" / "tl_loudness_tables.inc"
RATES = (48000, 44100, 32000, 24000, 22050, 16000)
# ITU-R BS.1770-4, tables 1 and 2 (48 kHz): b0 b1 b2 a1 a2 of the shelf, then of the high-pass
BS1770 = [1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585,
          1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621]


def _gen():
    spec = importlib.util.spec_from_file_location("gen_loudness_tables", ROOT / "tools" / "gen_loudness_tables.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _committed():
    """the arrays of the .inc as written: name -> float64 (hex floats read exactly)"""
    out = {}
    for name, body in re.findall(r"static const double (\w+)(?:\[\d+\])+ = \{(.*?)\};", INC.read_text(), flags=re.S):
        body = re.sub(r"//[^\n]*", "", body)
        out[name] = np.array([float.fromhex(v) for v in re.findall(r"-?0x[0-9a-f.]+p[+-]?\d+", body)])
    return out


def test_generator_reproduces_the_committed_table():
    assert _gen().text() == INC.read_text()


def test_the_48_khz_row_is_the_one_bs_1770_prints():
    t = _committed()
    assert t["tl_loudness_taps"].shape == (60,) and t["tl_loudness_edges"].shape == (751,) and t["tl_loudness_centres"].shape == (751,)
    err = np.abs(t["tl_loudness_taps"][:10] - np.array(BS1770)).max()
    print("largest difference from the printed coefficients: %.3g" % err)
    assert err <= 1e-12


def test_the_gating_scale_is_ordered():
    t = _committed()
    e, c = t["tl_loudness_edges"], t["tl_loudness_centres"]
    assert (np.diff(e) > 0).all()
    assert (e[:750] <= c[:750]).all() and (c[:750] < e[1:]).all() and c[750] >= e[750]
    assert e[0] == c[0] == 10.0 ** ((-70.0 + 0.691) / 10.0)
    assert abs(-0.691 + 10.0 * np.log10(c[470]) - (-23.0)) < 1e-9 and abs(-0.691 + 10.0 * np.log10(c[750]) - 5.0) < 1e-9


def test_the_library_returns_the_table():
    import odr_audioenc_amd as M
    if not M.LIB_PATH.exists():
        M.build()
    t = _committed()
    for i, r in enumerate(RATES):
        assert M.loudness_taps(r).tobytes() == t["tl_loudness_taps"][10 * i:10 * i + 10].tobytes(), r
    edges, centres = M.loudness_scale()
    assert edges.tobytes() == t["tl_loudness_edges"].tobytes() and centres.tobytes() == t["tl_loudness_centres"].tobytes()
    with pytest.raises(M.ToolameError) as e:
        M.loudness_taps(8000)
    assert e.value.code == 1
