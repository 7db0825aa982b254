"""The loudness meter's kernels as lane loops (tests/emu/mp2_loudness_emu.cpp: csrc/mp2_loudness.h with -DTL_EMULATE) against the
definition restated in numpy (loudnesslib.Oracle), bit for bit; then the anchors from the standards on the emulation alone (the long
signals are too slow for the oracle's Python loop): BS.1770-4's 997 Hz sine and EBU Tech 3341 cases 1 to 5; then the same emulation as a
program of its own under AddressSanitizer + UBSan."""
import math
import subprocess

import numpy as np
import pytest

import loudnesslib as LL

N = LL.N


@pytest.fixture(scope="module")
def pcm():
    return LL.pcm_of(LL.STREAMS)


@pytest.fixture(scope="module")
def oracle(pcm):
    """the oracle's records after every frame count at which some cut ends, and its programme at the end: computed once"""
    o = LL.Oracle(LL.STREAMS)
    ends = sorted({sum(c[:i + 1]) for c in LL.CUTS[0:1] + LL.CUTS[2:] for i in range(len(c))})
    recs, f0 = {}, 0
    for e in ends:
        recs[e] = o.loudness(pcm[f0:e])
        f0 = e
    return recs, o.programme(), o


def test_the_set_is_the_one_the_kernel_can_get_wrong():
    assert len(LL.STREAMS) == 37
    assert {(c["samplerate"], c["mode"]) for c in LL.STREAMS} == {(r, m) for r in LL.RATES for m in "sm"}
    assert LL.NFRAMES * N // 1600 >= 30 and LL.NFRAMES * N // 4800 >= 10


def test_oracle_sees_every_part_of_the_definition(oracle):
    recs, prog, _ = oracle
    r = recs[LL.NFRAMES]
    assert (r["frames"] == LL.NFRAMES).all()
    assert [int(b) for b in r["bins"]] == [LL.NFRAMES * N // (c["samplerate"] // 10) for c in LL.STREAMS]
    assert ((r["blocks"] == r["bins"] - 3)).all()
    assert (r["short_term"][r["bins"] >= 30] > 0).any() and (r["short_term"][r["bins"] < 30] == 0).all()
    silent = [s for s in range(37) if LL.KINDS[s % 7][0] == "silence"]
    assert (r["gated"][silent] == 0).all() and (prog["integrated"][silent] == 0).all()
    quiet = [s for s in range(37) if LL.KINDS[s % 7] == ("noise", -80.0)]
    assert (r["gated"][quiet] == 0).all() and (r["momentary"][quiet] > 0).all()      # measured, below the absolute gate
    loud = [s for s in range(37) if LL.KINDS[s % 7] == ("square", 0.0)]
    assert (r["gated"][loud] == r["blocks"][loud]).all() and (prog["gated"][loud] > 0).all()


@pytest.mark.parametrize("cuts", LL.CUTS, ids=["one", "frames", "7+38"])
def test_emulation_equals_the_definition(pcm, oracle, cuts):
    recs, prog, _ = oracle
    e = LL.LoudnessEmu(LL.STREAMS)
    f0 = 0
    for n in cuts:
        got = e.loudness(pcm[f0:f0 + n])
        f0 += n
        if f0 in recs:
            assert LL.same(got, recs[f0]), f0
    assert LL.same(e.programme(), prog)
    assert LL.same(e.rec, recs[LL.NFRAMES])


def test_reset_and_reconfigure_in_mid_run(pcm):
    """after 20 frames: stream 3 is reset, stream 8 (32 kHz stereo) becomes 16 kHz mono, all streams go on for 10 frames"""
    new = dict(samplerate=16000, mode="m")
    o, e = LL.Oracle(LL.STREAMS), LL.LoudnessEmu(LL.STREAMS)
    o.loudness(pcm[:20]); e.loudness(pcm[:20])
    for x in (o, e):
        x.reset(3)
        x.reconfigure(8, new)
    want, got = o.loudness(pcm[20:30]), e.loudness(pcm[20:30])
    assert LL.same(got, want)
    assert got["frames"][3] == 10 and got["frames"][8] == 10 and got["frames"][4] == 30
    assert got["bins"][8] == 10 * N // 1600
    assert LL.same(e.programme(), o.programme())
    o.reset(-1); e.reset(-1)
    assert LL.same(e.loudness(pcm[30:31]), o.loudness(pcm[30:31]))


def _measure(x, rate, nch):
    """x int16 [nch][n] through the emulation as ONE stream -> (record, programme record)"""
    nf = x.shape[1] // N
    p = np.zeros((nf, 1, 2, N), dtype=np.int16)
    p[:, 0, :nch] = x[:, :nf * N].reshape(nch, nf, N).transpose(1, 0, 2)
    e = LL.LoudnessEmu([dict(samplerate=rate, mode="m" if nch == 1 else "s")])
    r = e.loudness(p)
    return r[0], e.programme()[0]


@pytest.mark.parametrize("rate", LL.RATES)
def test_full_scale_997_hz_sine_in_one_channel_reads_minus_3_01(rate):
    """BS.1770-4: a 0 dBFS 997 Hz sine in one channel reads -3.01 LKFS.  The bilinear coefficient rows move that by up to 0.04 LU at
    the lowest rate (measured with these coefficients: -3.011 at 48 kHz down to -2.970 at 16 kHz), inside +-0.1 LU"""
    n = np.arange(3 * rate // N * N + N)
    x = np.round(32767.0 * np.sin(2.0 * math.pi * 997.0 * n / rate)).astype(np.int16)[None]
    r, p = _measure(x, rate, 1)
    for v in (r["momentary"], r["short_term"] if r["bins"] >= 30 else r["momentary"], p["integrated"]):
        assert abs(LL.lufs(float(v)) - (-3.01)) <= 0.1, (rate, LL.lufs(float(v)))


def _tones(parts, fs=48000):
    out, st = [], 0
    for db, sec in parts:
        n = np.arange(st, st + int(round(sec * fs)))
        s = np.round(32767.0 * 10.0 ** (db / 20.0) * np.sin(2.0 * math.pi * 1000.0 * n / fs))
        st += len(n)
        out.append(s)
    s = np.concatenate(out).astype(np.int16)
    return np.stack([s, s])


EBU = {1: ([(-23, 20)], -23.0), 2: ([(-33, 20)], -33.0), 3: ([(-36, 10), (-23, 60), (-36, 10)], -23.0),
       4: ([(-72, 10), (-36, 10), (-23, 60), (-36, 10), (-72, 10)], -23.0), 5: ([(-26, 20), (-20, 20.1), (-26, 20)], -23.0)}


@pytest.mark.parametrize("case", sorted(EBU))
def test_ebu_tech_3341_programme_loudness(case):
    """EBU Tech 3341 test signals 1 to 5, synthesised from their descriptions as 1 kHz stereo sines at 48 kHz: integrated loudness within the
    document's own +-0.1 LU.  (The definition alone gives -23.000, -33.000, -23.021, -23.021 and -22.985.)"""
    parts, want = EBU[case]
    _, p = _measure(_tones(parts), 48000, 2)
    got = LL.lufs(float(p["integrated"]))
    print("case %d: %.3f LUFS" % (case, got))
    assert abs(got - want) <= 0.1, got


def test_sanitized_program():
    """tests/emu/loudness_sanitize_main.cpp: the emulation over the 37-stream set and over 1, 31 and 33 streams under AddressSanitizer +
    UBSan, built and run as a program of its own"""
    exe = LL.build_sanitized()
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "sanitized ok" in r.stdout, (r.returncode, r.stdout, r.stderr[-2000:])
