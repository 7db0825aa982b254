"""Layer II feeds (csrc/mp2_feed.h over csrc/mp2_unpack.h and csrc/mp2_synth.h) on the lane-loop emulation, without a GPU: frames of the
oracle encoder, untouched and made foreign three ways, against a numpy statement of the standard, against the emulation's tlb_decode of
the same frames, against each other and under a call cut; hostile input, also as a program linked with AddressSanitizer + UBSan.  The
emulation libraries are compiled by this module into a temporary directory."""
import shutil

import numpy as np
import pytest

import declib as D
import feedlib as F

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")


@pytest.fixture(scope="module")
def feed_so(tmp_path_factory):
    return F.build_emu(tmp_path_factory.mktemp("feedemu"))


@pytest.fixture(scope="module")
def dec_so(tmp_path_factory):
    return D.build_emu(tmp_path_factory.mktemp("feeddecemu"))


_RUNS = {}


def run_case(feed_so, i):
    """case i once: the oracle's six frames, their four variants as four streams of one emulated feed call"""
    if i not in _RUNS:
        case = F.CASES[i]
        fcfg = F.feed_cfg_of(case)
        frames = F.oracle_frames(case, F.case_pcm(i, case))
        var = F.variants_of(frames, fcfg)
        e = F.FeedEmu(feed_so, [fcfg] * len(F.VARIANTS))
        assert e.stride == F.slot_bytes(fcfg)
        fr, ln = D.batch_arrays([var[v] for v in F.VARIANTS], e.stride)
        pcm, rep = e.decode(fr, ln)
        e.close()
        _RUNS[i] = dict(case=case, fcfg=fcfg, frames=frames, var=var, fr=fr, ln=ln, pcm=pcm, rep=rep)
    return _RUNS[i]


CASE_IDS = [f"{fs // 1000}k_{mode}_{kbps}" for fs, mode, kbps, _ in F.CASES]


def test_the_cases_are_the_ones_asked_for(feed_so):
    assert [c[:3] for c in F.CASES] == [(48000, "s", 192), (48000, "j", 128), (48000, "d", 64), (48000, "m", 64), (44100, "s", 128), (32000, "s", 384),
                                        (24000, "m", 32), (16000, "s", 64)]
    r = run_case(feed_so, 1)                                     # joint stereo: the frames do switch between stereo and joint stereo
    assert {b[3] >> 6 for b in r["frames"]} == {0, 1}
    r = run_case(feed_so, 4)                                     # 44.1 kHz: frames of both lengths
    assert len({len(b) for b in r["frames"]}) == 2
    assert len(run_case(feed_so, 5)["frames"][0]) == 1728        # the longest frame there is
    assert len(run_case(feed_so, 2)["frames"]) == F.NFRAMES


@pytest.mark.parametrize("i", range(len(F.CASES)), ids=CASE_IDS)
def test_reports_and_untouched_output(feed_so, i):
    """every variant of every frame passes, with the header's mode, the CRC-16 where there is one and the reader's bit count; nothing is
    written behind a one-channel feed's 1152 samples"""
    r = run_case(feed_so, i)
    nch = r["fcfg"]["channels"]
    for v, name in enumerate(F.VARIANTS):
        for f, fr in enumerate(r["var"][name]):
            rep = r["rep"][f, v]
            info = F.read_feed_frame(fr, r["fcfg"])
            assert int(rep["status"]) == 0, (name, f, hex(int(rep["status"])))
            assert (int(rep["mode"]), int(rep["mode_ext"])) == (fr[3] >> 6, (fr[3] >> 4) & 3)
            assert int(rep["audio_bits"]) == info["audio_bits"], (name, f)
            if name == "strip_crc":
                assert int(rep["crc_stored"]) == 0 and int(rep["crc_computed"]) == 0
            else:
                assert int(rep["crc_stored"]) == int(rep["crc_computed"]) == info["crc_computed"] == info["crc_stored"], (name, f)
    assert (r["pcm"][:, :, 1152 * nch:] == F.POISON).all()
    assert np.abs(r["pcm"][:, 0, :1152 * nch].astype(int)).max() > 1000          # audio, not silence


def test_pcm_equals_the_standards_flow_chart(feed_so):
    """(i) against the numpy statement, as test_decode_emu.test_pcm_equals_the_standards_flow_chart asks of tlb_decode_*: two fp64
    evaluations that differ only in summation order differ by about 1e-8 of an int16 step, so a rounding flip is rare but legal:
    |difference| <= 1 on at most 10 samples per million compared, 0 anywhere else.  Every case, every variant."""
    total = flips = 0
    for i in range(len(F.CASES)):
        r = run_case(feed_so, i)
        nch = r["fcfg"]["channels"]
        for v, name in enumerate(F.VARIANTS):
            want = F.numpy_feed_pcm(r["var"][name], r["fcfg"])[:, :1152 * nch]
            got = r["pcm"][:, v, :1152 * nch]
            d = np.abs(got.astype(np.int64) - want.astype(np.int64))
            assert d.max() <= 1, (CASE_IDS[i], name, int(d.max()))
            total += d.size
            flips += int((d != 0).sum())
    print(f"feed PCM vs numpy: {flips} rounding flips in {total} samples")
    assert flips * 1_000_000 <= 10 * total, (flips, total)


@pytest.mark.parametrize("i", range(len(F.CASES)), ids=CASE_IDS)
def test_untouched_frames_equal_tlb_decode(feed_so, dec_so, i):
    """(ii) the code is shared, so equality is the requirement: the feed's PCM of the untouched frames is the emulated tlb_decode's PCM of
    the same frames (under the ENCODER's configuration), re-interleaved"""
    r = run_case(feed_so, i)
    fs, mode, kbps, _ = r["case"]
    d = D.DecEmu(dec_so, [dict(samplerate=fs, mode=mode, kbps=kbps, psy=1)])
    fr, ln = D.batch_arrays([r["frames"]], d.stride)
    rep, _, pcm = d.decode(fr, ln, False, True)
    d.close()
    assert not (rep["status"] & D.BAD_MASK).any()
    nch = r["fcfg"]["channels"]
    assert np.array_equal(F.interleave(pcm[:, 0], nch)[:, :1152 * nch], r["pcm"][:, 0, :1152 * nch])


@pytest.mark.parametrize("i", range(len(F.CASES)), ids=CASE_IDS)
def test_all_variants_give_identical_pcm(feed_so, i):
    """(iii)"""
    r = run_case(feed_so, i)
    for v in range(1, len(F.VARIANTS)):
        assert np.array_equal(r["pcm"][:, v], r["pcm"][:, 0]), F.VARIANTS[v]


@pytest.mark.parametrize("i", range(len(F.CASES)), ids=CASE_IDS)
def test_a_cut_run_gives_the_same(feed_so, i):
    """(iv) 2 + 4 frames in two calls = 6 in one"""
    r = run_case(feed_so, i)
    e = F.FeedEmu(feed_so, [r["fcfg"]] * len(F.VARIANTS))
    a = e.decode(r["fr"][:2], r["ln"][:2])
    b = e.decode(r["fr"][2:], r["ln"][2:])
    e.close()
    assert np.array_equal(np.concatenate([a[0], b[0]]), r["pcm"]) and np.array_equal(np.concatenate([a[1], b[1]]), r["rep"])


def test_streams_without_a_feed_and_empty_slots(feed_so):
    """a stream without a feed: report EMPTY, its slots untouched; an empty slot of a fed stream: EMPTY, zeros, silence for its successor;
    feed_reset: the next frame is decoded as after silence"""
    r = run_case(feed_so, 0)
    fcfgs = [r["fcfg"], None, r["fcfg"]]
    e = F.FeedEmu(feed_so, fcfgs)
    slots = [[(b, len(b)) for b in r["frames"]] for _ in range(3)]
    slots[2][3] = (b"", 0)
    fr, ln = F.slots_to_arrays(slots, e.stride)
    pcm, rep = e.decode(fr, ln)
    assert np.array_equal(pcm[:, 0], r["pcm"][:, 0])
    assert (pcm[:, 1] == F.POISON).all() and (rep["status"][:, 1] == D.EMPTY).all()
    assert int(rep[3, 2]["status"]) == D.EMPTY and not pcm[3, 2].any()
    want = F.numpy_feed_pcm([None if f == 3 else b for f, b in enumerate(r["frames"])], r["fcfg"])
    assert np.abs(pcm[:, 2].astype(int) - want.astype(int)).max() <= 1
    assert not np.array_equal(pcm[4, 2], r["pcm"][4, 0]) and np.array_equal(pcm[5, 2], r["pcm"][5, 0])
    # reset of stream 0 between two calls: frame 2 as after silence, stream 2 as before
    e.reset()
    a = e.decode(fr[:2], ln[:2])
    e.reset(0)
    b = e.decode(fr[2:], ln[2:])
    e.close()
    assert np.array_equal(np.concatenate([a[0], b[0]])[:, 2], pcm[:, 2])
    want = F.numpy_feed_pcm(r["frames"][2:], r["fcfg"])
    assert np.abs(b[0][:, 0].astype(int) - want.astype(int)).max() <= 1 and not np.array_equal(b[0][0, 0], pcm[2, 0])


# ---- hostile input ---------------------------------------------------------------------------------------------------------------------
def hostile_batch(feed_so, i):
    """every hostile input of case i as one stream each of ONE feed call (stream 0: the good frames)"""
    r = run_case(feed_so, i)
    stride = F.slot_bytes(r["fcfg"])
    inputs = F.hostile_inputs(r["frames"], r["fcfg"], stride)
    slots = [[(b, len(b)) for b in r["frames"]]] + [sl for _, sl, _ in inputs]
    fr, ln = F.slots_to_arrays(slots, stride)
    return r, inputs, fr, ln


HOSTILE_CASES = list(range(len(F.CASES)))


@pytest.mark.parametrize("i", HOSTILE_CASES, ids=[CASE_IDS[i] for i in HOSTILE_CASES])
def test_hostile_input_is_flagged_and_contained(feed_so, i):
    """random bytes, a frame truncated at every 32nd byte, a wrong bitrate index, a wrong rate index, the wrong channel count, a bit_alloc
    field forced to all ones: the documented flag, never a ScF-CRC flag, zero PCM, the successor's history as after silence, nothing else
    changed"""
    r, inputs, fr, ln = hostile_batch(feed_so, i)
    names = [n for n, _, _ in inputs]
    assert {"random", "trunc32", "bitrate", "rate", "mode", "alloc"} <= set(names) and sum(n.startswith("trunc") for n in names) == (len(r["frames"][F.HOSTILE_SLOT]) - 1) // 32
    nch = r["fcfg"]["channels"]
    e = F.FeedEmu(feed_so, [r["fcfg"]] * fr.shape[1])
    pcm, rep = e.decode(fr, ln)
    e.close()
    assert np.array_equal(pcm[:, 0], r["pcm"][:, 0])
    h = F.HOSTILE_SLOT
    silent = [None if f == h else b for f, b in enumerate(r["frames"])]
    want = F.numpy_feed_pcm(silent, r["fcfg"])
    after_silence = None
    for k, (name, sl, must) in enumerate(inputs):
        s = k + 1
        st = int(rep[h, s]["status"])
        assert st & must and st & D.BAD_MASK, (name, hex(st))
        assert not st & (D.BAD_SCFCRC | D.SCFCRC_UNCHECKED | D.EMPTY), (name, hex(st))
        assert not pcm[h, s, :1152 * nch].any(), name            # a failed frame is 1152 zeros per channel
        keep = [f for f in range(F.NFRAMES) if f not in (h, h + 1)]
        assert np.array_equal(pcm[keep, s], r["pcm"][keep, 0]) and np.array_equal(rep[keep, s], r["rep"][keep, 0]), name
        if after_silence is None:
            after_silence = pcm[h + 1, s]
            assert np.abs(after_silence.astype(int)[:1152 * nch] - want[h + 1, :1152 * nch].astype(int)).max() <= 1
            if np.abs(r["pcm"][h, 0].astype(int)).max() > 100:               # (a damaged frame that was all but silent itself leaves the same history)
                assert not np.array_equal(after_silence, r["pcm"][h + 1, 0])
        assert np.array_equal(pcm[h + 1, s], after_silence), name  # the successor's history is silence, whatever the damage was
    assert any(int(rep[h, k + 1]["status"]) & D.OVERRUN for k, n in enumerate(names) if n.startswith("trunc"))


def test_hostile_lengths_and_noise_stay_inside_the_slot(feed_so):
    """random bytes and all-ones bytes under every kind of length, from below 0 to beyond the stride: flags and zeros"""
    fcfgs = [F.feed_cfg_of(c) for c in F.CASES]
    e = F.FeedEmu(feed_so, fcfgs)
    fr, ln = noise_case(len(fcfgs), e.stride)
    pcm, rep = e.decode(fr, ln)
    e.close()
    assert (rep["status"][ln > 0] & D.BAD_MASK).all() and (rep["status"][ln <= 0] == D.EMPTY).all()
    assert not pcm[F.expected_written(pcm, fcfgs)].any() and (pcm[~F.expected_written(pcm, fcfgs)] == F.POISON).all()


def noise_case(ns, stride):
    rng = np.random.default_rng(5)
    fr = rng.integers(0, 256, (6, ns, stride), dtype=np.uint8)
    fr[1] = 0xff
    fr[2, :, :4] = [0xff, 0xfc, 0xf0, 0xff]
    ln = rng.integers(0, stride + 40, (6, ns)).astype(np.int32)
    ln[3] = -5
    return fr, ln


def test_hostile_input_is_clean_under_asan_ubsan(tmp_path, feed_so):
    """the same hostile sets, and the noise, through the lane-loop build linked as a program with AddressSanitizer + UBSan
    (tests/emu/mp2_feed_san_main.cpp; its buffers are exactly as long as the data).  Clean, and the same reports and PCM as the plain
    build, whose flags the tests above have checked."""
    exe = F.build_san_driver(tmp_path)
    for i in HOSTILE_CASES:
        r, inputs, fr, ln = hostile_batch(feed_so, i)
        fcfgs = [r["fcfg"]] * fr.shape[1]
        (rep, pcm), = F.run_san_driver(exe, tmp_path, fcfgs, [(fr, ln)])
        e = F.FeedEmu(feed_so, fcfgs)
        want_pcm, want_rep = e.decode(fr, ln)
        e.close()
        assert rep.tobytes() == want_rep.tobytes() and pcm.tobytes() == want_pcm.tobytes(), CASE_IDS[i]
    fcfgs = [F.feed_cfg_of(c) for c in F.CASES] + [None]
    e = F.FeedEmu(feed_so, fcfgs)
    fr, ln = noise_case(len(fcfgs), e.stride)
    (rep, pcm), = F.run_san_driver(exe, tmp_path, fcfgs, [(fr, ln)])
    want_pcm, want_rep = e.decode(fr, ln)
    e.close()
    assert rep.tobytes() == want_rep.tobytes() and pcm.tobytes() == want_pcm.tobytes()
