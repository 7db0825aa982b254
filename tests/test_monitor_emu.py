"""The confidence monitor's fold (csrc/mp2_monitor.h) on the lane-loop emulation, without a GPU, against the rule of
include/toolame_batch.h written as a plain Python loop (tests/monitorlib.py fold_python): (a) random reports over every status flag with
random PCM, (b) reports and PCM of the decode emulation on golden frames, some with a damaged byte, (c) the same slots in one call and
in pieces, (d) without PCM, (e) the duration a silent frame adds at each of the six sample rates against the oracle's silence counter.
The emulation library is compiled by this module into a temporary directory."""
import shutil

import numpy as np
import pytest

import declib as D
import monitorlib as ML
import oraclelib as O

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")
RATES = (48000, 32000, 24000, 16000, 44100, 22050)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return ML.MonitorEmu(ML.build_emu(tmp_path_factory.mktemp("monitoremu")))


def _same(got, want, what=""):
    for k in ML.RECORD_DTYPE.names:
        assert np.array_equal(got[k], want[k]), (what, k, got[k], want[k])


def _random_case(seed, nf=23, ns=13):
    """ns is no multiple of 4; status words over all eight flags (about a third of the slots EMPTY, a third clean); PCM random with
    stretches of all-zero and all-negative frames; stream 1 all zero, stream 2 all negative, streams 3 and 7 mono (channel 1 zero)"""
    rng = np.random.default_rng(seed)
    status = rng.integers(0, 256, size=(nf, ns))
    kind = rng.integers(0, 3, size=(nf, ns))
    status = np.where(kind == 0, status | D.EMPTY, np.where(kind == 1, status & D.SCFCRC_UNCHECKED, status & ~D.EMPTY))
    pcm = rng.integers(-32768, 32768, size=(nf, ns, 2, 1152)).astype(np.int16)
    quiet = rng.integers(0, 4, size=(nf, ns))
    pcm[quiet == 0] = 0
    pcm[quiet == 1] = -np.abs(pcm[quiet == 1].astype(np.int32)).clip(1, 32768).astype(np.int16)
    one = rng.integers(0, 2, size=(nf, ns)).astype(bool)             # one channel silent, the other not
    pcm[one & (quiet == 2), 1] = 0
    pcm[:, 1] = 0
    pcm[:, 2] = -np.abs(pcm[:, 2].astype(np.int32)).clip(1, 32768).astype(np.int16)
    pcm[:, 3, 1] = 0
    pcm[:, 7, 1] = 0
    pcm[5, 4] = -32768                                               # the extremes, and a lone positive sample in the last word of each channel
    pcm[6, 4] = -5
    pcm[6, 4, 0, 1151] = 1
    pcm[7, 4] = -5
    pcm[7, 4, 1, 1151] = 32767
    status[5:8, 4] = 0
    rates = [RATES[s % 6] for s in range(ns)]
    nch = [1 if s in (3, 7) else 2 for s in range(ns)]
    return status, pcm, rates, nch


def test_record_layout(emu):
    assert ML.RECORD_DTYPE.itemsize == 32
    assert [ML.RECORD_DTYPE.fields[k][1] for k in ML.RECORD_DTYPE.names] == [0, 4, 8, 12, 16, 20, 24, 28]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_reports_and_pcm_equal_the_python_loop(emu, seed):
    """case (a); the record starts from zero and, a second time, from a record that is not zero"""
    status, pcm, rates, nch = _random_case(seed)
    assert all((status & (1 << b)).any() for b in range(8))
    rec = np.zeros(status.shape[1], dtype=ML.RECORD_DTYPE)
    emu.fold(ML.reports_of(status), pcm, rates, nch, rec)
    want = ML.fold_python(status, pcm, rates)
    _same(rec, want, "from zero")
    assert want["out_silence_ms"].any() and want["bad_run"].any() and (want["out_peak"] > 0).any()
    assert want["out_silence_ms"][1] > 0 and want["out_silence_ms"][2] > 0 and not want["out_peak"][1].any() and not want["out_peak"][2].any()
    status2, pcm2, _, _ = _random_case(seed + 100)
    emu.fold(ML.reports_of(status2), pcm2, rates, nch, rec)
    _same(rec, ML.fold_python(status2, pcm2, rates, want), "carried on")


def test_split_into_calls_gives_identical_records(emu):
    """case (c): one call, and pieces of 1, 2, 3 ... frames"""
    status, pcm, rates, nch = _random_case(7, nf=21)
    whole = np.zeros(status.shape[1], dtype=ML.RECORD_DTYPE)
    emu.fold(ML.reports_of(status), pcm, rates, nch, whole)
    parts = np.zeros_like(whole)
    f, k = 0, 1
    while f < status.shape[0]:
        emu.fold(ML.reports_of(status[f:f + k]), pcm[f:f + k], rates, nch, parts)
        f, k = f + k, k + 1
    assert f >= status.shape[0] and k > 5
    _same(parts, whole)
    ones = np.zeros_like(whole)
    for f in range(status.shape[0]):
        emu.fold(ML.reports_of(status[f:f + 1]), pcm[f:f + 1], rates, nch, ones)
    _same(ones, whole)


def test_without_pcm_peaks_and_silence_stay(emu):
    """case (d): out_peak and out_silence_ms are untouched (an EMPTY slot still zeroes the peaks: step 2 of the rule comes first)"""
    status, pcm, rates, nch = _random_case(11)
    rec = np.zeros(status.shape[1], dtype=ML.RECORD_DTYPE)
    emu.fold(ML.reports_of(status[:8]), pcm[:8], rates, nch, rec)    # something to keep
    before = rec.copy()
    assert before["out_silence_ms"].any() and before["out_peak"].any()
    noempty = status[8:] & ~D.EMPTY
    emu.fold(ML.reports_of(noempty), None, rates, nch, rec)
    _same(rec, ML.fold_python(noempty, None, rates, before))
    assert np.array_equal(rec["out_peak"], before["out_peak"]) and np.array_equal(rec["out_silence_ms"], before["out_silence_ms"])
    assert not np.array_equal(rec["frames"], before["frames"])
    emu.fold(ML.reports_of(status[8:]), None, rates, nch, rec)
    _same(rec, ML.fold_python(status[8:], None, rates, ML.fold_python(noempty, None, rates, before)))
    assert np.array_equal(rec["out_silence_ms"], before["out_silence_ms"])


def test_silent_frame_duration_equals_the_silence_oracle(emu):
    """case (e): one stream at each rate, stereo and mono; k silent frames add what the oracle's silence counter (mp2o_silence_ms, the
    reference's arithmetic) adds for zero peaks, and a frame with audio resets both"""
    L = O.lib()
    for nchan in (2, 1):
        ns, nf = len(RATES), 5
        pcm = np.zeros((nf, ns, 2, 1152), dtype=np.int16)
        pcm[3, :, 0, 17] = 9                                         # frame 3 has audio
        rec = np.zeros(ns, dtype=ML.RECORD_DTYPE)
        want = [0] * ns
        for f in range(nf):
            emu.fold(ML.reports_of(np.zeros((1, ns), dtype=int)), pcm[f:f + 1], RATES, [nchan] * ns, rec)
            for s, fs in enumerate(RATES):
                pk = np.array([max(0, int(pcm[f, s, 0].max())), max(0, int(pcm[f, s, 1].max()))], dtype=np.int16)
                want[s] = L.mp2o_silence_ms(want[s], pk.ctypes.data, nchan, fs)
            assert [int(x) for x in rec["out_silence_ms"]] == want, (nchan, f)
        assert want == [1000 * 1152 // fs for fs in RATES] and want[0] == 24 and want[4] == 26


@pytest.fixture(scope="module")
def dec_so(tmp_path_factory):
    return D.build_emu(tmp_path_factory.mktemp("decemu_mon"))


def test_decoded_golden_frames_with_damage(emu, dec_so):
    """case (b): 13 goldens over the rates and modes as one batch through the decode emulation, single bytes damaged in some frames;
    the fold of its reports and PCM equals the Python loop, whole and in two calls (the decoder itself is split the same way)"""
    names = D.golden_names()
    gs = [np.load(D.GOLDEN / (n + ".npz")) for n in names]
    cfgs = [D.golden_cfg(g) for g in gs]
    pick, seen = [], set()
    for i, c in enumerate(cfgs):                                     # the first golden of every (rate, mode), at most 13
        key = (c["samplerate"], c["mode"])
        if key not in seen and len(pick) < 13:
            seen.add(key)
            pick.append(i)
    assert len(pick) >= 6 and len({cfgs[i]["samplerate"] for i in pick}) >= 3
    cfgs = [cfgs[i] for i in pick]
    frames = [D.cut_frames(gs[i]["data"], c) for i, c in zip(pick, cfgs)]
    e = D.DecEmu(dec_so, cfgs)
    fr, ln = D.batch_arrays(frames, e.stride)
    rng = np.random.default_rng(5)
    hit = []
    for s in range(0, len(cfgs), 2):                                 # every other stream: one byte of two of its frames
        for k, f in enumerate(sorted(rng.choice(np.arange(1, len(frames[s])), size=2, replace=False))):
            b = int(rng.integers(4, 6)) if k == 0 else int(rng.integers(0, ln[f, s]))      # the stored CRC-16 (always noticed), then any byte
            fr[f, s, b] ^= 1 << int(rng.integers(0, 8))
            hit.append((int(f), s))
    cut = fr.shape[0] // 2
    rep1, _, pcm1 = e.decode(fr[:cut], ln[:cut], False, True)
    rep2, _, pcm2 = e.decode(fr[cut:], ln[cut:], False, True)
    e.close()
    rep, pcm = np.concatenate([rep1, rep2]), np.concatenate([pcm1, pcm2])
    rates = [c["samplerate"] for c in cfgs]
    nch = [1 if c["mode"] == "m" else 2 for c in cfgs]
    want = ML.fold_python(rep["status"], pcm, rates)
    assert (want["bad_frames"][0::2] >= 1).all() and (want["bad_frames"][1::2] == 0).all()
    assert (want["flags_seen"] & D.SCFCRC_UNCHECKED).all() and (want["out_peak"] > 0).any()
    whole = np.zeros(len(cfgs), dtype=ML.RECORD_DTYPE)
    emu.fold(rep, pcm, rates, nch, whole)
    _same(whole, want)
    two = np.zeros(len(cfgs), dtype=ML.RECORD_DTYPE)
    emu.fold(rep1, pcm1, rates, nch, two)
    emu.fold(rep2, pcm2, rates, nch, two)
    _same(two, want)
