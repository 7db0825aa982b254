"""Ingest with short reads (csrc/mp2_ingest.h) on the lane-loop emulation, without a GPU: against the output of the reference's own
expand_missing_samples on a ramp (tests/golden/short_reads.npz), against a numpy statement of the three cases on random PCM with junk
behind `valid`, against the existing ingest path where every read is full, the underrun counters against a plain loop and the silence
counter against the oracle.  The emulation library is compiled by this module into a temporary directory."""
import ctypes as C
import re
import shutil
from pathlib import Path

import numpy as np
import pytest

import ingestlib as I
import oraclelib as O

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")
ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ["tlb_ingest_device_valid", "tlb_ingest_host_valid", "tlb_underrun_device", "tlb_underrun_host", "tlb_tick_enable_short_reads",
               "tlb_tick_valid", "tlb_tick_underrun_ms", "tlb_tick_underruns", "tlb_node_enable_short_reads", "tlb_node_valid",
               "tlb_node_underrun_ms", "tlb_node_underruns"]


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return I.IngestEmu(I.build_emu(tmp_path_factory.mktemp("ingestemu")))


def _ramp():
    """L = i + 1, R = -(i + 1): the output of the stretch is the index map"""
    i = np.arange(I.FRAMES, dtype=np.int16) + 1
    st = np.stack([i, -i], axis=1).reshape(-1)
    mo = np.zeros(2 * I.FRAMES, dtype=np.int16)
    mo[:I.FRAMES] = i
    return st, mo


def test_fixture_covers_the_cases_the_issue_names():
    valid, st, mo = I.fixture()
    want = sorted(set(range(1152 - 130, 1153)) | {0, 1, 500, 1000})
    assert list(valid) == want and st.shape == (len(want), 1152, 2) and mo.shape == (len(want), 1152)


def test_emulation_equals_the_reference_on_the_ramp(emu):
    """every fixture case, stereo and mono, as one batch of (case, stream) slots; the caller's buffer holds junk behind `valid`"""
    valid, st, mo = I.fixture()
    n = len(valid)
    ramp_s, ramp_m = _ramp()
    inter = np.zeros((n, 2, 2 * I.FRAMES), dtype=np.int16)
    inter[:, 0] = ramp_s
    inter[:, 1] = ramp_m
    for k, v in enumerate(valid):                                    # junk where the queue would have left zeros
        inter[k, 0, 2 * v:] = 0x7abc
        inter[k, 1, v:] = 0x7abc
    v2 = np.stack([valid, valid], axis=1).astype(np.int32)
    pcm, peaks = emu.ingest(inter, v2, [2, 1], [0.0, 0.0])
    for k, v in enumerate(valid):
        assert np.array_equal(pcm[k, 0, 0], st[k, :, 0]) and np.array_equal(pcm[k, 0, 1], st[k, :, 1]), int(v)
        assert np.array_equal(pcm[k, 1, 0], mo[k]) and not pcm[k, 1, 1].any(), int(v)
        assert peaks[k, 0, 0] == st[k, :, 0].max() and peaks[k, 0, 1] == 0, int(v)
        assert peaks[k, 1, 0] == max(int(mo[k, 0::2].max()), 0) and peaks[k, 1, 1] == max(int(mo[k, 1::2].max()), 0), int(v)
    # the two consequences the header states: one missing frame ends on a zero of the tail, 105 missing frames drop 22 valid ones
    k1, k105 = list(valid).index(1151), list(valid).index(1152 - 105)
    assert st[k1, -1, 0] == 0 and st[k1, -2, 0] == 1151
    assert st[k105, :, 0].max() == (1152 - 105) - 22
    # 115 missing frames are stretched, 116 are not
    assert st[list(valid).index(1152 - 115), 20, 0] != 21 and np.array_equal(st[list(valid).index(1152 - 116), :1036, 0], np.arange(1036) + 1)


def test_numpy_statement_equals_the_reference_on_the_ramp():
    """the checker itself (ingestlib.stretch) against the fixture, so that the random test below stands on the reference too"""
    valid, st, mo = I.fixture()
    ramp_s, ramp_m = _ramp()
    for k, v in enumerate(valid):
        assert np.array_equal(I.stretch(ramp_s, v, 2).reshape(1152, 2), st[k]), int(v)
        assert np.array_equal(I.stretch(ramp_m, v, 1)[:1152], mo[k]), int(v)


def _random_case(seed, nf, valid_pool):
    rng = np.random.default_rng(seed)
    nch = [2, 1, 2, 1, 2, 2, 1]
    gains = [0.0, 0.0, -3.5, 6.0, 2.25, -12.0, 0.5]
    ns = len(nch)
    inter = rng.integers(-32768, 32768, size=(nf, ns, 2 * I.FRAMES), dtype=np.int64).astype(np.int16)
    inter[np.abs(inter) < 3] = 77                                    # no zeros by chance: a zero in the output is a zero of the tail
    valid = rng.choice(valid_pool, size=(nf, ns)).astype(np.int32)
    return inter, valid, nch, gains


def test_random_pcm_gain_and_junk_behind_valid(emu):
    """random PCM, non-zero gains, non-zero junk behind `valid`: the emulation equals the numpy statement, the junk never shows, and the
    peaks are the peaks of the stretched buffer"""
    fx = I.fixture()[0]
    pool = np.concatenate([fx, fx, [1152] * 40, [-5, 1153, 2000, 1 << 30, -(1 << 31)]])
    inter, valid, nch, gains = _random_case(11, 60, pool)
    pcm, peaks = emu.ingest(inter, valid, nch, gains)
    want_pcm, want_pk = I.ingest_numpy(inter, valid, nch, gains)
    assert np.array_equal(pcm, want_pcm) and np.array_equal(peaks, want_pk)
    # a second run whose junk differs: only the bytes behind `valid` change, so the output must not
    junk = inter.copy()
    for f in range(inter.shape[0]):
        for s in range(inter.shape[1]):
            v = min(max(int(valid[f, s]), 0), 1152)
            junk[f, s, (2 * v if nch[s] == 2 else v):] ^= 0x5a5a
    pcm2, peaks2 = emu.ingest(junk, valid, nch, gains)
    assert np.array_equal(pcm2, pcm) and np.array_equal(peaks2, peaks)
    # the tail of a short slot is zero: sample frames behind the last live output frame
    for f in range(0, inter.shape[0], 7):
        for s in range(inter.shape[1]):
            _, live = I.src_index(valid[f, s])
            dead = ~live
            assert not pcm[f, s, 0][dead].any() and not pcm[f, s, 1][dead].any()
            if nch[s] == 2 and gains[s] == 0.0:
                assert (pcm[f, s, 0][live] != 0).all()


def test_full_reads_are_the_existing_ingest_path(emu):
    """every `valid` at 1152, at 2000, or no array at all: byte-equal to the existing ingest (the oracle's mp2o_ingest, which the device's
    tl_ingest_kernel is held to by tests/test_hip_parity.py)"""
    inter, _, nch, gains = _random_case(5, 9, [1152])
    nf, ns = inter.shape[:2]
    L = O.lib()
    want = np.zeros((nf, ns, 2, I.FRAMES), dtype=np.int16)
    want_pk = np.zeros((nf, ns, 2), dtype=np.int16)
    for f in range(nf):
        for s in range(ns):
            src = np.ascontiguousarray(inter[f, s])
            out = np.zeros((2, I.FRAMES), dtype=np.int16)
            pk = np.zeros(2, dtype=np.int16)
            L.mp2o_ingest(src.ctypes.data, nch[s], gains[s], out.ctypes.data, pk.ctypes.data)
            want[f, s], want_pk[f, s] = out, pk
    for valid in (np.full((nf, ns), 1152, np.int32), np.full((nf, ns), 2000, np.int32), None):
        pcm, peaks = emu.ingest(inter, valid, nch, gains)
        assert pcm.tobytes() == want.tobytes() and peaks.tobytes() == want_pk.tobytes()


@pytest.mark.parametrize("rate", [48000, 24000, 16000])
def test_underrun_counters(emu, rate):
    """a random short / full pattern in ragged calls (the cuts of tests/test_decode_emu.py) against a plain loop"""
    rng = np.random.default_rng(rate)
    ns, nf = 9, 16
    rates = [rate] * ns
    nch = [2 if s % 3 else 1 for s in range(ns)]
    valid = np.where(rng.random((nf, ns)) < 0.4, rng.integers(-3, 1152, size=(nf, ns)), rng.choice([1152, 1153, 4000], size=(nf, ns))).astype(np.int32)
    valid[:, 0] = 1152                                               # never short
    valid[:, 1] = 1151                                               # always short
    valid[:-1, 2] = 7; valid[-1, 2] = 1152                           # a full read at the end resets the time, not the count
    ms, n = np.zeros(ns, np.uint32), np.zeros(ns, np.uint32)
    pos = 0
    for cut in (1, 7, 3, 2, 1, 2):
        emu.underrun(valid[pos:pos + cut], rates, nch, ms, n)
        pos += cut
    assert pos == nf
    want_ms, want_n = I.underrun_python(valid, rates, [0] * ns, [0] * ns)
    assert list(ms) == want_ms and list(n) == want_n
    per = {48000: 24, 24000: 48, 16000: 72}[rate]
    assert ms[0] == 0 and n[0] == 0 and ms[1] == nf * per and n[1] == nf and ms[2] == 0 and n[2] == nf - 1
    one_ms, one_n = np.zeros(ns, np.uint32), np.zeros(ns, np.uint32)
    emu.underrun(valid, rates, nch, one_ms, one_n)
    assert np.array_equal(one_ms, ms) and np.array_equal(one_n, n)


def test_silence_counter_every_rate(emu):
    """the silence counter (tl_silence_stream, what tl_silence_kernel runs) against the oracle's mp2o_silence_ms frame by frame: all six
    rates with two channels and with one, counters that do not start at 0, in ragged calls and one frame a call"""
    L = O.lib()
    rates, nch, peaks, start = I.silence_case()
    nf, ns = peaks.shape[:2]
    want = np.zeros((nf + 1, ns), dtype=np.uint32)                   # want[f]: the counters before frame f
    want[0] = start
    for f in range(nf):
        for s in range(ns):
            want[f + 1, s] = L.mp2o_silence_ms(int(want[f, s]), np.ascontiguousarray(peaks[f, s]).ctypes.data, nch[s], rates[s])
    assert [int(x) for x in want[nf]] == I.silence_python(peaks, rates, start)
    ms, pos = start.copy(), 0
    for cut in I.SILENCE_CUTS:
        emu.silence(peaks[pos:pos + cut], rates, nch, ms)
        pos += cut
        assert np.array_equal(ms, want[pos]), pos
    assert pos == nf
    ms = start.copy()
    for f in range(nf):
        emu.silence(peaks[f:f + 1], rates, nch, ms)
        assert np.array_equal(ms, want[f + 1]), f
    # the columns: always silent, never silent, one frame with audio last, peaks (0, 3) once in the middle
    per = [int(L.mp2o_silence_ms(0, np.zeros(2, np.int16).ctypes.data, nch[s], rates[s])) for s in range(ns)]
    for s in range(ns):
        col = s % 4
        assert ms[s] == (int(start[s]) + nf * per[s], 0, 0, (nf - 1 - nf // 2) * per[s])[col], s
        step = np.zeros(1, np.uint32)
        emu.silence(np.zeros((1, 1, 2), np.int16), rates[s:s + 1], nch[s:s + 1], step)
        assert step[0] == per[s], s
        if rates[s] != 22050:                                        # 22.05 kHz: whatever the oracle returns
            assert per[s] == {48000: 24, 32000: 36, 24000: 48, 16000: 72, 44100: 26}[rates[s]], s


def test_new_symbols_are_declared_exported_and_loadable():
    import subprocess
    import odr_audioenc_amd as M
    src = (ROOT / "include" / "toolame_batch.h").read_text()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    declared = set(re.findall(r"\b(tlb_[a-z0-9_]+)\s*\(", src))
    if not M.LIB_PATH.exists():
        M.build()
    out = subprocess.run(["nm", "-D", "--defined-only", str(M.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split()}
    lib = C.CDLL(str(M.LIB_PATH))
    for name in NEW_SYMBOLS:
        assert name in declared and name in exported and hasattr(lib, name), name
    # the kernels are in the library's gfx950 code objects, and the existing ingest kernel is still there beside them
    import json
    js = ROOT / "build" / "isa" / "short_reads_summary.json"
    r = subprocess.run([__import__("sys").executable, str(ROOT / "tools" / "check_isa.py"), str(M.LIB_PATH), "--json", str(js)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    summary = json.loads(js.read_text())
    for k in ("tl_ingest_valid_kernel", "tl_underrun_kernel", "tl_ingest_kernel"):
        assert any(k in name for name in summary), k
    v = [rec for name, rec in summary.items() if "tl_ingest_valid_kernel" in name]
    assert len(v) == 1 and v[0]["vgpr_spill"] == 0 and v[0]["sgpr_spill"] == 0 and v[0]["scratch"] == 0
    # the Python surface
    assert all(hasattr(M.Tick, a) for a in ("enable_short_reads", "valid", "underrun_ms", "underruns"))
    assert all(hasattr(M.Node, a) for a in ("enable_short_reads", "valid", "underrun_ms", "underruns"))
    import inspect
    assert "valid" in inspect.signature(M.Batch.ingest).parameters
