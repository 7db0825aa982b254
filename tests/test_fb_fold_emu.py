"""The filterbank's folded operand table (csrc/mp2_fb.h, csrc/mp2_host.cpp tl_build_tables), CPU only: the premise of the proof in
mp2_fb.h on the golden window, the table as raw bits against a numpy restatement, and the kernel source through the lane-loop
emulation against the oracle on signals whose window sums are exact zeros or single products (tests/fbfoldlib.py)."""
import shutil
import subprocess

import numpy as np
import pytest

import emulib as E
import fbfoldlib as F


@pytest.fixture(scope="module")
def enwindow(golden_dir):
    return np.load(golden_dir / "tables_48k.npz")["enwindow"]


def test_no_window_row_has_eight_coefficients_of_no_positive_sign(enwindow):
    """ta = -0.0 needs eight products of -0.0: eight zero samples on eight coefficients <= 0.  No row of the window is like that, so
    ta + (a zero of either sign) is ta bit for bit -- checked on the table the reference's taps pin, not trusted."""
    rows = enwindow.reshape(8, 64).T                            # row r: coefficients r, r + 64, ... r + 448
    positives = (rows > 0).sum(axis=1)
    print("positive coefficients per row, min:", int(positives.min()), "at row", int(positives.argmin()))
    assert rows.shape == (64, 8) and (positives >= 1).all()
    assert np.array_equal(np.rint(rows[16] * 1e9).astype(np.int64), [-2384, 69618, -21458, -4756451, 30526638, 4638195, 747204, 49591])


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")
def test_operand_table_is_the_folded_window_bit_for_bit(enwindow, tmp_path):
    """tl_build_tables() is the one builder: tests/emu/Makefile links csrc/mp2_host.cpp into the emulation, csrc/Makefile into the
    product.  Its enwindow stays the golden window; its enwindow_s is window / 32768 with rows 49..63 negated and row 48 +0.0."""
    exe = tmp_path / "fb_table_main"
    csrc = E.ROOT / "odr-audioenc_amd" / "csrc"
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-fno-strict-aliasing", "-Wno-unknown-pragmas", "-o", str(exe),
                        str(E.EMU_DIR / "fb_table_main.cpp"), str(csrc / "mp2_host.cpp"), "-lm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    raw = subprocess.run([str(exe)], capture_output=True, timeout=120)
    assert raw.returncode == 0 and len(raw.stdout) == 2 * 512 * 8
    got = np.frombuffer(raw.stdout, dtype=np.float64).reshape(2, 512)
    assert np.array_equal(got[0].view(np.uint64), enwindow.view(np.uint64))
    want = F.folded_table(enwindow)
    assert np.array_equal(got[1].view(np.uint64), want.view(np.uint64))
    row = np.arange(512) & 63
    assert (got[1][row == 48].view(np.uint64) == 0).all()                                  # +0.0, not -0.0
    flipped = row > 48
    assert np.array_equal(got[1][flipped], -(enwindow[flipped] / 32768.0)) and np.array_equal(got[1][row < 48], enwindow[row < 48] / 32768.0)


@pytest.mark.parametrize("cfg_name", [n for n, _ in F.CONFIGS])
def test_emulation_equals_oracle_on_zero_sum_signals(cfg_name):
    cfg = dict(F.CONFIGS)[cfg_name]
    pcm = F.batch_pcm()
    b = E.EmuBatch([cfg] * pcm.shape[1])
    got, taps = b.encode(pcm, want_taps=True)
    tail = b.flush()
    b.close()
    zeros = F.check_against_oracle(cfg_name, got, tail, taps)
    print(cfg_name, "streams:", pcm.shape[1], "sb_sample words that are a zero of either sign:", zeros)
    assert zeros > 0
    if cfg["mode"] == "m":
        # a launch with taps runs every stream alone; without them the mono streams of one configuration share waves in pairs
        # (tl_encode_pair: the filterbank with channel 0 of two streams on its lane halves): the same bytes
        b = E.EmuBatch([cfg] * pcm.shape[1])
        got2, _ = b.encode(pcm)
        tail2 = b.flush()
        pairs = b.pair_units()
        b.close()
        assert pairs == (pcm.shape[1] // 2) * F.NFRAMES
        assert [g + t for g, t in zip(got2, tail2)] == [r for r, _ in F.oracle(cfg_name)]
