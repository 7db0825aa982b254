"""The loudness range's kernels as lane loops (tests/emu/mp2_lra_emu.cpp: csrc/mp2_loudness.h with -DTL_EMULATE) against the definition
restated in Python (lralib.Oracle, lralib.range_rule), bit for bit on counts and records; the counting wave against the plain one on
everything the loudness meter reports; tl_lra_range on constructed histograms at the rule's boundaries; EBU Tech 3342's synthetic cases 1
to 4 on the emulation alone (the long signals are too slow for the oracle's Python loop); then the same emulation as a program of its own
under AddressSanitizer + UBSan."""
import math
import subprocess

import numpy as np
import pytest

import loudnesslib as LL
import lralib as RL

N = RL.N


@pytest.fixture(scope="module")
def pcm():
    return RL.pcm_of(RL.ORACLE_STREAMS, RL.ORACLE_NFRAMES)


@pytest.fixture(scope="module")
def oracle(pcm):
    """the oracle over the whole signal, computed once: loudness records, range counts and range records at the end"""
    o = RL.Oracle(RL.ORACLE_STREAMS)
    rec = o.loudness(pcm)
    return rec, o.hist_st.copy(), o.lra(), o.programme()


def test_the_set_is_the_one_the_kernel_can_get_wrong(oracle):
    rec, hist_st, lra, _ = oracle
    assert {(c["samplerate"], c["mode"]) for c in RL.ORACLE_STREAMS} == {(r, m) for r in LL.RATES for m in "sm"}
    bins = [RL.ORACLE_NFRAMES * N // (c["samplerate"] // 10) for c in RL.ORACLE_STREAMS]
    assert [int(b) for b in rec["bins"]] == bins and min(bins) >= 33
    live = [s for s in range(13) if s not in (RL.SILENT, RL.QUIET)]
    assert [int(hist_st[s].sum()) for s in live] == [bins[s] - 29 for s in live]          # one range block per bin from bin 30 on
    assert not hist_st[RL.SILENT].any() and not hist_st[RL.QUIET].any() and rec["short_term"][RL.QUIET] > 0
    assert (lra["blocks"][live] == hist_st[live].sum(axis=1)).all() and (lra["gated"][live] >= 1).all()
    assert (lra["high_bin"] > lra["low_bin"]).any()
    for s in (RL.SILENT, RL.QUIET):
        assert lra[s].tobytes() == bytes(40)


@pytest.mark.parametrize("cuts", RL.ORACLE_CUTS, ids=["one", "frames", "7+133", "64+13+63"])
def test_emulation_equals_the_definition(pcm, oracle, cuts):
    rec, hist_st, lra, prog = oracle
    e = RL.LraEmu(RL.ORACLE_STREAMS)
    got = LL.run_cuts(e, pcm, cuts)[-1]
    assert RL.same(got, rec) and RL.same(e.rec, rec)
    assert (e.hist_st[:RL.NBINS].T.astype(np.int64) == hist_st).all() and not e.hist_st[RL.NBINS:].any()
    assert RL.same(e.lra(), lra)
    assert RL.same(e.programme(), prog)


@pytest.mark.parametrize("cuts", RL.ORACLE_CUTS[:3], ids=["one", "frames", "7+133"])
def test_counting_wave_reports_what_the_plain_one_reports(pcm, cuts):
    a, b = RL.LraEmu(RL.ORACLE_STREAMS, counting=True), RL.LraEmu(RL.ORACLE_STREAMS, counting=False)
    f0 = 0
    for n in cuts:
        assert RL.same(a.loudness(pcm[f0:f0 + n]), b.loudness(pcm[f0:f0 + n]))
        f0 += n
    for x in ("lane", "ring", "hist"):
        assert getattr(a, x).tobytes() == getattr(b, x).tobytes(), x
    assert RL.same(a.rec, b.rec) and RL.same(a.programme(), b.programme())
    assert a.hist_st.any() and not b.hist_st.any()
    plain = LL.LoudnessEmu(RL.ORACLE_STREAMS)                         # ... and what tests/emu/mp2_loudness_emu.cpp, untouched, reports
    plain.loudness(pcm)
    assert RL.same(plain.rec, a.rec) and plain.hist.tobytes() == a.hist.tobytes() and plain.lane.tobytes() == a.lane.tobytes()


def test_reset_and_reconfigure_in_mid_run(pcm):
    """after 90 frames: stream 3 is reset, stream 8 (32 kHz stereo) becomes 16 kHz mono, all streams go on for 50 frames"""
    new = dict(samplerate=16000, mode="m")
    o, e = RL.Oracle(RL.ORACLE_STREAMS), RL.LraEmu(RL.ORACLE_STREAMS)
    o.loudness(pcm[:90]); e.loudness(pcm[:90])
    assert e.hist_st[:, 3].any() and e.hist_st[:, 8].any()
    for x in (o, e):
        x.reset(3)
        x.reconfigure(8, new)
    assert RL.same(e.loudness(pcm[90:140]), o.loudness(pcm[90:140]))
    assert RL.same(e.lra(), o.lra())
    assert e.lra()["blocks"][3] == 0 and e.lra()["blocks"][8] == 50 * N // 1600 - 29 and e.lra()["blocks"][4] > 0


def _hist(**bins):
    h = [0] * RL.NBINS
    for j, n in bins.items():
        h[int(j[1:])] = n
    return h


def _cases():
    c = {"empty": _hist(), "one block": _hist(b417=1), "all in one bin": _hist(b300=977), "last bin": _hist(b750=3), "first bin": _hist(b0=5)}
    for n2 in (2, 10, 11, 20, 21):                                   # the rank boundaries: one block a bin, so the ranks are the bins
        c["N2 = %d" % n2] = _hist(**{"b%d" % (400 + 3 * i): 1 for i in range(n2)})
        c["N2 = %d uneven" % n2] = _hist(**{"b%d" % (200 + 7 * i): (2 if i == n2 // 3 else 1) for i in range(n2 - 1)})
    c["near 2^32"] = _hist(b100=2147483647, b700=2147483647, b701=1)
    c["near 2^32 in one"] = _hist(b333=4294967295)
    c["relative gate cuts"] = _hist(b50=40, b60=40, b400=300, b450=300, b500=291)
    return c


def test_range_rule_on_constructed_histograms():
    """tl_lra_range = the rule on Python ints, on the rule's own boundaries; the expected figures of a few are written out by hand"""
    centres = LL.tables()[2]
    cases = _cases()
    names, hists = list(cases), list(cases.values())
    want = RL.records_of(hists)
    got = RL.emu_range(hists)
    for i, k in enumerate(names):
        assert got[i].tobytes() == want[i].tobytes(), (k, got[i], want[i])
    r = dict(zip(names, want))
    assert r["empty"].tobytes() == bytes(40)
    assert (r["one block"]["blocks"], r["one block"]["gated"], r["one block"]["low_bin"], r["one block"]["high_bin"]) == (1, 1, 417, 417)
    assert r["one block"]["low"] == centres[417] == r["one block"]["high"] and r["one block"]["gate"] == np.float64(0.01) * (centres[417] / np.float64(1.0))
    assert (r["all in one bin"]["low_bin"], r["all in one bin"]["high_bin"], r["all in one bin"]["gated"]) == (300, 300, 977)
    # one block a bin at 400 + 3 i: ranks r_lo = (N2 + 4) // 10 and r_hi = (19 (N2 - 1) + 10) // 20 are 0-based positions
    for n2, lo, hi in ((2, 0, 1), (10, 1, 9), (11, 1, 10), (20, 2, 18), (21, 2, 19)):
        x = r["N2 = %d" % n2]
        assert (int(x["gated"]), int(x["low_bin"]), int(x["high_bin"])) == (n2, 400 + 3 * lo, 400 + 3 * hi), n2
        assert lo == math.floor((n2 - 1) * 0.10 + 0.5) and hi == math.floor((n2 - 1) * 0.95 + 0.5)
    x = r["near 2^32"]
    assert (int(x["blocks"]), int(x["gated"]), int(x["low_bin"]), int(x["high_bin"])) == (4294967295, 2147483648, 700, 700)      # the crowd at bin 100 is 60 LU down: gated out
    x = r["near 2^32 in one"]
    assert (int(x["gated"]), int(x["low_bin"]), int(x["high_bin"])) == (4294967295, 333, 333) and 19 * (4294967295 - 1) > 2 ** 32
    x = r["relative gate cuts"]
    assert (int(x["blocks"]), int(x["gated"])) == (971, 891) and RL.lu(x) == 10.0


def test_gate_on_a_centre_is_kept():
    """c_k >= gate with gate == c_k bit for bit: bin k belongs to the distribution.  0.01 * c_200 is c_0 in the committed table, and with
    2 013 077 blocks in bin 0, 2 in bin 200 and 85 559 906 in bin 201 (a convergent of (c_201 - c_200) / (c_200 - c_0)) the rounded mean
    is c_200 itself: the gate falls on the centre of an occupied bin, and its blocks count.  With 1 or 4 blocks in bin 200 the mean rounds
    elsewhere; whichever side the gate then falls, both sides must decide alike."""
    centres = LL.tables()[2]
    assert np.float64(0.01) * centres[200] == centres[0]
    h = _hist(b0=2013077, b200=2, b201=85559906)
    want, got = RL.records_of([h])[0], RL.emu_range([h])[0]
    assert want["gate"] == centres[0] and int(want["blocks"]) == int(want["gated"]) == 2013077 + 2 + 85559906
    assert (int(want["low_bin"]), int(want["high_bin"])) == (201, 201)
    assert got.tobytes() == want.tobytes()
    gated = set()
    for n in (1, 4, 11, 13):
        h = _hist(b0=2013077, b200=n, b201=85559906)
        want, got = RL.records_of([h])[0], RL.emu_range([h])[0]
        assert got.tobytes() == want.tobytes(), n
        gated.add(int(want["blocks"]) - int(want["gated"]))
    print("blocks below the gate in the neighbouring histograms:", sorted(gated))


def _tones(parts, fs=48000):
    out, st = [], 0
    for db, sec in parts:
        n = np.arange(st, st + int(round(sec * fs)))
        out.append(np.round(32767.0 * 10.0 ** (db / 20.0) * np.sin(2.0 * math.pi * 1000.0 * n / fs)))
        st += len(n)
    s = np.concatenate(out).astype(np.int16)
    return np.stack([s, s])


TECH3342 = {1: ([(-20, 20), (-30, 20)], 10.0), 2: ([(-20, 20), (-15, 20)], 5.0), 3: ([(-40, 20), (-20, 20)], 20.0),
            4: ([(-50, 20), (-35, 20), (-20, 20), (-35, 20), (-50, 20)], 15.0)}


@pytest.mark.parametrize("case", sorted(TECH3342))
def test_ebu_tech_3342_loudness_range(case):
    """EBU Tech 3342 synthetic test signals 1 to 4 from their descriptions: 1 kHz stereo sines at 48 kHz in 20 s segments, the level in
    dBFS peak per channel = LUFS (a stereo sine at -23 dBFS reads -23 LUFS: Tech 3341 case 1).  LRA within the document's own +-1 LU."""
    parts, want = TECH3342[case]
    x = _tones(parts)
    nf = x.shape[1] // N
    p = np.zeros((nf, 1, 2, N), dtype=np.int16)
    p[:, 0] = x[:, :nf * N].reshape(2, nf, N).transpose(1, 0, 2)
    e = RL.LraEmu([dict(samplerate=48000, mode="s")])
    e.loudness(p)
    r = e.lra()[0]
    print("case %d: LRA %.1f LU, %.2f .. %.2f LUFS, gate %.2f, %d of %d blocks" % (case, RL.lu(r), LL.lufs(float(r["low"])), LL.lufs(float(r["high"])),
                                                                                   LL.lufs(float(r["gate"])), r["gated"], r["blocks"]))
    assert abs(RL.lu(r) - want) <= 1.0, RL.lu(r)


def test_sanitized_program():
    """tests/emu/lra_sanitize_main.cpp: the counting wave and tl_lra_range over the 37-stream set and over 1, 31 and 33 streams under
    AddressSanitizer + UBSan, built and run as a program of its own"""
    exe = RL.build_sanitized()
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "sanitized ok" in r.stdout, (r.returncode, r.stdout, r.stderr[-2000:])
