"""The compare monitor's kernel (csrc/mp2_compare.h) on the lane-loop emulation, without a GPU, against the definitions of
include/toolame_batch.h written as a plain Python-int loop (tests/comparelib.py Oracle).  The frames come from the encoder emulation and
the decoded PCM from the decode emulation, which the goldens pin: six streams (stereo, joint, dual, a mono pair, LSF), six frames and the
flush.  Records are compared byte for byte: one call, ragged cuts, the NULL-input flush, exchanged / swapped / zeroed decoded PCM, a slot
with a BAD report, a history reset; and the delay itself is measured here.  The emulation libraries are compiled by this module into a
temporary directory."""
import re
import shutil
from pathlib import Path

import numpy as np
import pytest

import comparelib as CL
import declib as D
import emulib as E

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")
ROOT = Path(__file__).resolve().parent.parent
NF = 6
NCH = [CL.nch_of(c) for c in CL.STREAMS]
P = CL.PARAMS


def _encode_decode(cfgs, pcm, dec_so):
    """-> (report [nf + 1][ns], dec [nf + 1][ns][2][1152]): the call's slots, then the flushed frames as one more slot"""
    nf = pcm.shape[0]
    e = E.EmuBatch([dict(c, psy=1) for c in cfgs])
    out = np.zeros((nf + 1, e.n, e.stride), dtype=np.uint8)
    lens = np.zeros((nf + 1, e.n), dtype=np.int32)
    e.L.emu_encode_len(e.h, np.ascontiguousarray(pcm).ctypes.data, nf, None, None, out.ctypes.data, e.stride, None, lens.ctypes.data)
    for s, fr in enumerate(e.flush()):
        out[nf, s, :len(fr)] = np.frombuffer(fr, dtype=np.uint8)
        lens[nf, s] = len(fr)
    e.close()
    d = D.DecEmu(dec_so, cfgs)
    assert d.stride == out.shape[2]
    rep, _, dec = d.decode(out, lens, False, True)
    d.close()
    return rep, dec


@pytest.fixture(scope="module")
def dec_so(tmp_path_factory):
    return D.build_emu(tmp_path_factory.mktemp("decemu_cmp"))


@pytest.fixture(scope="module")
def cmp_so(tmp_path_factory):
    return CL.build_emu(tmp_path_factory.mktemp("compareemu"))


@pytest.fixture(scope="module")
def run(dec_so):
    """the shared, undisturbed run: pcm [NF], reports and decoded PCM [NF + 1] (the last slot is the flush), the oracle's records and sums"""
    pcm = CL.noise(NF, len(CL.STREAMS))
    rep, dec = _encode_decode(CL.STREAMS, pcm, dec_so)
    st = rep["status"].astype(int)
    assert (st[0] == D.EMPTY).all() and not (st[1:] & (D.EMPTY | D.BAD_MASK)).any()
    o = CL.Oracle(NCH)
    want, seen = o.compare(pcm, dec[:NF], st[:NF], P)
    want_f, seen_f = o.compare(None, dec[NF:], st[NF:], P, want)
    for a in (pcm, rep, dec, want, want_f):
        a.setflags(write=False)
    return dict(pcm=pcm, rep=rep, dec=dec, st=st, want=want, want_f=want_f, seen=seen + [(NF, *r[1:]) for r in seen_f])


def _emu(cmp_so):
    return CL.CompareEmu(cmp_so, NCH)


def test_inputs_meet_the_conditions(run):
    """every compared frame of every stream is judged, healthy correlation >= 3/4, mispaired <= 1/4 -- on the oracle's sums, so that no
    test below can pass by sitting on the threshold"""
    CL.check_input_conditions(run["seen"], CL.mispaired_sums(run["pcm"], run["dec"][:NF], NCH), set(range(len(NCH))))
    w = run["want_f"]
    assert (w["frames_compared"] == NF).all() and (w["frames_judged"] == NF).all() and not w["mismatch_frames"].any() and not w["swapped_frames"].any()
    assert (w["last_flags"] == np.array([3, 3, 3, 1, 1, 1])).all()


def test_one_call_and_the_flush_equal_the_oracle(run, cmp_so):
    e = _emu(cmp_so)
    rec = e.compare(run["pcm"], run["dec"][:NF], run["rep"][:NF], P)
    CL.same(rec, run["want"], "one call")
    assert (rec["frames_compared"] == NF - 1).all()
    hist = e.hist.copy()
    e.compare(None, run["dec"][NF:], run["rep"][NF:], P, rec)
    CL.same(rec, run["want_f"], "flush")
    assert np.array_equal(hist, e.hist)                              # the NULL-input form does not advance the history


def test_ragged_cuts_give_identical_records(run, cmp_so):
    e = _emu(cmp_so)
    rec = np.zeros(len(NCH), dtype=CL.RECORD_DTYPE)
    pos = 0
    for cut in (1, 3, 2):
        assert e.compare(run["pcm"][pos:pos + cut], run["dec"][pos:pos + cut], run["rep"][pos:pos + cut], P, rec) is rec
        pos += cut
    assert pos == NF
    CL.same(rec, run["want"], "1 + 3 + 2")
    e.compare(None, run["dec"][NF:], run["rep"][NF:], P, rec)
    CL.same(rec, run["want_f"], "1 + 3 + 2 + flush")


def test_the_delay_is_measured(dec_so, cmp_so):
    """white noise through 48 kHz stereo, 24 kHz mono and a joint-stereo stream: over all lags 0..1151 of sum in * dec the largest is at
    the same lag for all, and that lag is TLB_COMPARE_DELAY of the header, of the kernel and of the Python binding"""
    cfgs = [dict(samplerate=48000, mode="s", kbps=192), dict(samplerate=24000, mode="m", kbps=64), dict(samplerate=48000, mode="j", kbps=128)]
    nf = 4
    pcm = CL.white(nf, len(cfgs))
    rep, dec = _encode_decode(cfgs, pcm, dec_so)
    lags = []
    for s, c in enumerate(cfgs):
        for ch in range(CL.nch_of(c)):
            x, f = pcm[:, s, ch].reshape(-1).astype(np.int64), 3
            y = dec[f, s, ch].astype(np.int64)                       # the audio of input frame f - 1
            sums = [int((x[(f - 1) * 1152 - lag:f * 1152 - lag] * y).sum()) for lag in range(1152)]
            lags.append(int(np.argmax(sums)))
    assert len(lags) == 5 and len(set(lags)) == 1, lags
    header = (ROOT / "include" / "toolame_batch.h").read_text()
    assert int(re.search(r"#define\s+TLB_COMPARE_DELAY\s+(\d+)", header).group(1)) == lags[0] == CL.DELAY
    assert _emu(cmp_so).L.cmp_delay() == lags[0]
    import odr_audioenc_amd as M
    assert M.COMPARE_DELAY == lags[0]


def test_a_quiet_stream_is_never_judged_and_never_a_mismatch(dec_so, cmp_so):
    """amplitude below min_energy (rms about 120 of the 256 that min_energy asks for), its decoded audio even exchanged with another's"""
    cfgs = [CL.STREAMS[0], CL.STREAMS[3]]
    pcm = (CL.noise(4, 2, seed=77) >> 6).astype(np.int16)
    rep, dec = _encode_decode(cfgs, pcm, dec_so)
    nch = [2, 1]
    dec = dec[:4, ::-1].copy()                                       # stream 0 hears stream 1 and the other way round
    want, seen = CL.Oracle(nch).compare(pcm, dec, rep["status"][:4], P)
    assert all(max(sxx) < P[0] and max(sxx) > 0 for f, s, sxx, _, _, _ in seen if f >= 2)
    rec = CL.CompareEmu(cmp_so, nch).compare(pcm, dec, rep[:4], P)
    CL.same(rec, want)
    assert (rec["frames_compared"] == 3).all() and not rec["frames_judged"].any() and not rec["mismatch_frames"].any() and not rec["last_flags"].any()


def test_two_streams_exchanged_mismatch_and_no_other_record_moves(run, cmp_so):
    """decoded PCM of the two streams of the mono pair exchanged on the host before the call: exactly those two mismatch, in every frame"""
    dec = run["dec"][:NF].copy()
    dec[:, [3, 4]] = dec[:, [4, 3]]
    want, _ = CL.Oracle(NCH).compare(run["pcm"], dec, run["st"][:NF], P)
    rec = _emu(cmp_so).compare(run["pcm"], dec, run["rep"][:NF], P)
    CL.same(rec, want)
    assert list(rec["mismatch_frames"]) == [0, 0, 0, NF - 1, NF - 1, 0] and list(rec["mismatch_run"]) == [0, 0, 0, NF - 1, NF - 1, 0]
    assert (rec["last_flags"][[3, 4]] == (CL.JUDGED0 | CL.MISMATCH)).all() and not rec["swapped_frames"].any()
    for s in (0, 1, 2, 5):
        assert rec[s].tobytes() == run["want"][s].tobytes()


def test_swapped_channels_are_counted(run, cmp_so):
    """left and right of the stereo stream exchanged: every frame a mismatch that matches crosswise"""
    dec = run["dec"][:NF].copy()
    dec[:, 0] = dec[:, 0, ::-1]
    want, _ = CL.Oracle(NCH).compare(run["pcm"], dec, run["st"][:NF], P)
    rec = _emu(cmp_so).compare(run["pcm"], dec, run["rep"][:NF], P)
    CL.same(rec, want)
    assert rec["swapped_frames"][0] == NF - 1 == rec["mismatch_frames"][0] and rec["last_flags"][0] == 15
    assert not rec["swapped_frames"][1:].any() and not rec["mismatch_frames"][1:].any()
    assert list(rec["sxz"][0]) == list(run["want"]["sxy"][0]) and list(rec["sxy"][0]) == list(run["want"]["sxz"][0])


def test_zeroed_decode_is_a_mismatch(run, cmp_so):
    dec = run["dec"][:NF].copy()
    dec[:, 2] = 0
    want, _ = CL.Oracle(NCH).compare(run["pcm"], dec, run["st"][:NF], P)
    rec = _emu(cmp_so).compare(run["pcm"], dec, run["rep"][:NF], P)
    CL.same(rec, want)
    assert list(rec["mismatch_frames"]) == [0, 0, NF - 1, 0, 0, 0] and not rec["syy"][2].any() and not rec["swapped_frames"].any()


def test_a_bad_slot_is_skipped_and_the_next_still_aligns(run, cmp_so):
    """slot 3 of stream 1 reports BAD_CRC16 (its decoded PCM is zeros then): not compared, its input still advances the history, so slot 4
    is a match again; with the bad slot LAST in a call the flags say SKIPPED and the sums are those of the slot before"""
    rep, dec = run["rep"][:NF].copy(), run["dec"][:NF].copy()
    rep["status"][3, 1] |= D.BAD_CRC16
    dec[3, 1] = 0
    o, e = CL.Oracle(NCH), _emu(cmp_so)
    want, _ = o.compare(run["pcm"][:4], dec[:4], rep["status"][:4], P)
    rec = e.compare(run["pcm"][:4], dec[:4], rep[:4], P)
    CL.same(rec, want, "bad slot last")
    assert rec["last_flags"][1] == CL.SKIPPED and rec["frames_compared"][1] == 2 and list(rec["sxx"][1]) == [r for r in run["seen"] if r[:2] == (2, 1)][0][2]
    want, _ = o.compare(run["pcm"][4:], dec[4:], rep["status"][4:], P, want)
    e.compare(run["pcm"][4:], dec[4:], rep[4:], P, rec)
    CL.same(rec, want, "the slots after it")
    assert rec["frames_compared"][1] == NF - 2 and rec["frames_judged"][1] == NF - 2 and not rec["mismatch_frames"].any()
    assert rec[1]["sxy"].tolist() == run["want"][1]["sxy"].tolist()  # the last slot's sums are those of the undisturbed run: it aligned


def test_a_zeroed_history_between_calls_is_never_judged(run, cmp_so):
    """What the kernel makes of the state the life-cycle calls leave (here the history the test holds for the emulation is zeroed by hand;
    the calls themselves -- tlb_stream_reset / _finish / _reconfigure, tlb_reset -- run in tests/test_compare_gpu.py): the stream's next
    slot has nothing to be set against (never judged), the slot after that only the frame that went in since; the others are untouched"""
    o, e = CL.Oracle(NCH), _emu(cmp_so)
    want, _ = o.compare(run["pcm"][:3], run["dec"][:3], run["st"][:3], P)
    rec = e.compare(run["pcm"][:3], run["dec"][:3], run["rep"][:3], P)
    o.reset(0)
    e.reset(0)
    want, seen = o.compare(run["pcm"][3:], run["dec"][3:NF], run["st"][3:NF], P, want)
    e.compare(run["pcm"][3:], run["dec"][3:NF], run["rep"][3:NF], P, rec)
    CL.same(rec, want)
    assert [r[2] for r in seen if r[:2] == (0, 0)] == [[0, 0]] and rec["frames_judged"][0] == NF - 2 and rec["frames_compared"][0] == NF - 1
    for s in range(1, len(NCH)):
        assert rec[s].tobytes() == run["want"][s].tobytes()
