"""Frame check and decode (csrc/mp2_unpack.h, csrc/mp2_synth.h) on the lane-loop emulation, without a GPU: against the reference's own
taps in every golden, against an independent bit-level reader, under damage, against a numpy statement of the standard's synthesis,
as a round trip, and under ragged call cuts.  The emulation library is compiled by this module into a temporary directory."""
import os
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import declib as D
import oraclelib as O
from pcmgen import gen_pcm

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")
ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def emu_so(tmp_path_factory):
    return D.build_emu(tmp_path_factory.mktemp("decemu"))


@pytest.fixture(scope="module")
def goldens():
    names = D.golden_names()
    assert len(names) == 126                                     # no golden may be left out
    gs = [np.load(D.GOLDEN / (n + ".npz")) for n in names]
    cfgs = [D.golden_cfg(g) for g in gs]
    frames = [D.cut_frames(g["data"], c) for g, c in zip(gs, cfgs)]
    assert all(len(f) == c["nframes"] for f, c in zip(frames, cfgs))
    return names, gs, cfgs, frames


@pytest.fixture(scope="module")
def golden_run(emu_so, goldens):
    """all 126 goldens as ONE mixed batch: reports, fields, PCM"""
    names, gs, cfgs, frames = goldens
    e = D.DecEmu(emu_so, cfgs)
    fr, ln = D.batch_arrays(frames, e.stride)
    rep, fl, pcm = e.decode(fr, ln, True, True)
    bad = e.bad_frames()
    e.close()
    return rep, fl, pcm, bad


def _own_mask(info, ba):
    """cells whose samples the frame transmits: an allocation, and channel 1 only below the joint-stereo bound"""
    m = ba != 0
    m[1, info["jsbound"]:] = False
    m[info["nch"]:] = False
    return m


def _oracle_subband(g, cfg):
    """the oracle's quantiser output per frame (tests/oraclelib.py, itself pinned to the reference)"""
    pcm = gen_pcm(cfg["seed"], cfg["kind"], 0, cfg["nframes"])
    e = O.OracleEncoder(samplerate=cfg["samplerate"], mode=cfg["mode"], kbps=cfg["kbps"], psy=cfg["psy"], pad_len=cfg["pad_len"])
    out = []
    for i in range(cfg["nframes"]):
        if "xpad" in g:
            e.encode(pcm[i], bytes(g["xpad"][i]), int(g["xpad_len"][i]))
        else:
            e.encode(pcm[i])
        out.append(e.taps()["subband"])
    e.close()
    return out


def test_fields_equal_the_reference_taps(goldens, golden_run):
    """Item 1.  bit_alloc over every (channel, subband) of the stream; scfsi and scalar where the frame transmits them (an allocation:
    the reference computes scalefactors for cells it then does not send, and no reader can get those back); subband where the frame
    transmits samples (an allocation, channel 1 below the bound only).  Exact equality."""
    names, gs, cfgs, frames = goldens
    rep, fl, _, bad = golden_run
    assert bad == 0
    cells = 0
    for s, (name, g, cfg) in enumerate(zip(names, gs, cfgs)):
        nch = 1 if cfg["mode"] == "m" else 2
        big = {int(f): i for i, f in enumerate(g["big_tap_frames"])} if "subband" in g else None
        osub = None if big is not None else _oracle_subband(g, cfg)
        for f in range(cfg["nframes"]):
            r, x = rep[f, s], fl[f, s]
            assert int(r["status"]) == (D.SCFCRC_UNCHECKED if f == 0 else 0), (name, f, hex(int(r["status"])))
            assert (int(r["mode"]), int(r["mode_ext"])) == (int(g["mode"][f]), int(g["mode_ext"][f])), (name, f)
            assert np.array_equal(x["bit_alloc"][:nch], g["bit_alloc"][f][:nch]), (name, f)
            m = x["bit_alloc"] != 0
            assert not m[nch:].any()
            assert np.array_equal(x["scfsi"][m], g["scfsi"][f][m]), (name, f)
            m3 = np.broadcast_to(m[:, None, :], (2, 3, 32))
            assert np.array_equal(x["scalar"][m3], g["scalar"][f][m3]), (name, f)
            info = D.read_frame(frames[s][f], cfg) if (big is None or f in big) else None
            if info is not None:
                want = g["subband"][big[f]] if big is not None else osub[f]
                ms = np.broadcast_to(_own_mask(info, x["bit_alloc"].astype(int))[:, None, None, :], (2, 3, 12, 32))
                cells += int(ms.sum())
                assert np.array_equal(x["subband"][ms].astype(np.int64), np.asarray(want)[ms].astype(np.int64)), (name, f)
    assert cells > 1_000_000                                     # (a digital-silence frame transmits none; the set as a whole does)


def test_crcs_equal_an_independent_reader(goldens, golden_run):
    """Item 2.  CRC-16 and ScF-CRC of every golden frame recomputed by tests/declib.py read_frame (plain Python over np.unpackbits) agree with
    the device path's crc_computed / crc_stored and flags; so do the fields it reads."""
    names, gs, cfgs, frames = goldens
    rep, fl, _, _ = golden_run
    for s, (name, cfg) in enumerate(zip(names, cfgs)):
        for f, fr in enumerate(frames[s]):
            info = D.read_frame(fr, cfg)
            r = rep[f, s]
            assert info["crc_computed"] == int(r["crc_computed"]) == info["crc_stored"] == int(r["crc_stored"]), (name, f)
            assert info["audio_bits"] == int(r["audio_bits"]), (name, f)
            # the reader's own verdict on the ScF-CRC: this frame's scalefactors against the tail of the frame before
            if f > 0:
                assert info["scfcrc"] == D.stored_scfcrc(frames[s][f - 1], cfg), (name, f)
                assert not int(r["status"]) & (D.BAD_SCFCRC | D.SCFCRC_UNCHECKED)
            for k in ("bit_alloc", "scfsi", "scalar", "subband"):
                assert np.array_equal(info[k], fl[f, s][k].astype(int)), (name, f, k)
        assert D.read_frame(frames[s][-1], cfg)["scfcrc"] == D.stored_scfcrc(frames[s][-1], cfg), name      # the last frame carries its own


# ---- item 3: damage ------------------------------------------------------------------------------------------------------------------
DAMAGE_STREAMS = ["p1_48k_s_128_k0", "p1_48k_j_128_k0", "p3_24k_m_64_k0", "p2_48k_d_128_k0", "p1_44k_j_192_k0", "p0_32k_m_64_k0",
                  "p1_16k_m_32_k0", "p4_48k_s_192_k0", "p1_48k_m_32_xpad80", "p3_22k_j_96_k0"]


def damage_cases(frame_lists, cfgs):
    """-> [(name, stream, frame, fn(bytearray) -> new length or None, flags that must be set, flags that are all that may be set)].
    Field positions come from the independent reader.  The scalefactor bit is the MOST significant bit of the first transmitted
    scalefactor of the lowest subband with an allocation in a band group the stream's ScF-CRC covers (groups 0..dab_ext-1: subbands
    0..3, 4..7, 8..15, 16..29): the ScF-CRC protects the three MSBs only, and scalefactors are outside the CRC-16."""
    cases = []
    for k, kind in enumerate(("header", "alloc", "scfsi", "scf", "sync", "trunc")):
        s = k % len(frame_lists)
        f = 3 + k
        cfg, fr = cfgs[s], frame_lists[s][f]
        info = D.read_frame(fr, cfg)
        T = D._tables()
        n_ba = sum(int(T["nbal"][T["line"][info["tab"]][sb]]) * (info["nch"] if sb < info["jsbound"] else 1) for sb in range(info["sblimit"]))
        n_sel = 2 * int((info["bit_alloc"][:info["nch"]] != 0).sum())

        def flip(bit):
            def fn(b):
                b[bit >> 3] ^= 0x80 >> (bit & 7)
            return fn
        if kind == "header":
            cases.append((kind, s, f, flip(16 + 1), D.HEADER_MISMATCH | D.BAD_CRC16, D.HEADER_MISMATCH | D.BAD_CRC16))      # a bitrate-index bit
        elif kind == "alloc":
            cases.append((kind, s, f, flip(48 + 1), D.BAD_CRC16, D.BAD_MASK))           # every later field moves: more flags may follow
        elif kind == "scfsi":
            cases.append((kind, s, f, flip(48 + n_ba + 1), D.BAD_CRC16, D.BAD_MASK))
        elif kind == "scf":
            assert info["bit_alloc"][0][0] != 0                                         # subband 0, channel 0 is transmitted: group 0, always covered
            cases.append((kind, s, f, flip(48 + n_ba + n_sel), D.BAD_SCFCRC, D.BAD_SCFCRC))
        elif kind == "sync":
            cases.append((kind, s, f, flip(3), D.BAD_SYNC, D.BAD_SYNC))
        else:
            # the LAST frame of the stream: a truncated frame has lost the tail that carries its successor's ScF-CRC, so a successor would
            # rightly turn SCFCRC_UNCHECKED (test_truncation_unchecks_the_successor); here no other frame may change at all
            f = len(frame_lists[s]) - 1
            cases.append((kind, s, f, lambda b: len(b) - 7, D.OVERRUN, D.OVERRUN))
    return cases


def run_damage(dec_factory, frame_lists, cfgs):
    """every case on a fresh decoder; returns nothing, asserts"""
    e = dec_factory(cfgs)
    fr0, ln0 = D.batch_arrays(frame_lists, e.stride)
    rep0, fl0, pcm0 = e.decode(fr0, ln0, True, True)
    e.close()
    assert not (rep0["status"] & D.BAD_MASK).any()
    for kind, s, f, fn, must, may in damage_cases(frame_lists, cfgs):
        fr, ln = fr0.copy(), ln0.copy()
        b = bytearray(fr[f, s, :ln[f, s]].tobytes())
        n = fn(b)
        fr[f, s, :len(b)] = np.frombuffer(bytes(b), dtype=np.uint8)
        if n is not None:
            ln[f, s] = n
        e = dec_factory(cfgs)
        rep, fl, pcm = e.decode(fr, ln, True, True)
        assert e.bad_frames() == 1, kind
        e.close()
        st = int(rep[f, s]["status"])
        assert st & must == must and not st & D.BAD_MASK & ~may, (kind, hex(st))
        assert not pcm[f, s].any(), kind                                                   # a failed frame is 1152 zeros per channel
        keep = np.ones(rep.shape, dtype=bool)
        keep[f, s] = False
        assert np.array_equal(rep[keep], rep0[keep]) and np.array_equal(fl[keep], fl0[keep]), kind
        keep[min(f + 1, rep.shape[0] - 1), s] = False                                      # its successor's filter history is now silence
        assert np.array_equal(pcm[keep], pcm0[keep]), kind


def _damage_set(goldens):
    names, gs, cfgs, frames = goldens
    idx = [names.index(n) for n in DAMAGE_STREAMS]
    return [frames[i] for i in idx], [cfgs[i] for i in idx]


def test_damage_is_found_and_contained(emu_so, goldens):
    """Item 3: exactly the damaged frame raises the expected flag; every other frame's report and fields equal the undamaged run."""
    fl, cfgs = _damage_set(goldens)
    assert len(cfgs) >= 8
    run_damage(lambda c: D.DecEmu(emu_so, c), fl, cfgs)


def run_truncation(dec_factory, fl, cfgs, f=5, s=2):
    """frame f of stream s loses its last 3 bytes; asserts"""
    e = dec_factory(cfgs)
    fr, ln = D.batch_arrays(fl, e.stride)
    rep0, _, _ = e.decode(fr, ln)
    e.close()
    ln[f, s] -= 3
    e = dec_factory(cfgs)
    rep, _, _ = e.decode(fr, ln)
    e.close()
    assert int(rep[f, s]["status"]) == D.OVERRUN and int(rep[f + 1, s]["status"]) == D.SCFCRC_UNCHECKED
    keep = np.ones(rep.shape, dtype=bool)
    keep[f:f + 2, s] = False
    assert np.array_equal(rep[keep], rep0[keep])


def test_truncation_unchecks_the_successor(emu_so, goldens):
    """A frame cut short in the MIDDLE of a stream: OVERRUN on it, SCFCRC_UNCHECKED (not an error) on the next frame, whose ScF-CRC bytes
    went with the lost tail; nothing else changes."""
    fl, cfgs = _damage_set(goldens)
    run_truncation(lambda c: D.DecEmu(emu_so, c), fl, cfgs)


def test_padding_bit_damage_unchecks_the_successor(emu_so, goldens):
    """44.1 kHz: a flipped padding bit makes the frame one byte longer or shorter than its slot.  The frame itself is flagged (CRC-16, and
    HEADER_MISMATCH or OVERRUN for the length); where its tail lies can no longer be trusted, so the NEXT frame is SCFCRC_UNCHECKED, not
    falsely BAD_SCFCRC; nothing else changes."""
    fl, cfgs = _damage_set(goldens)
    s = DAMAGE_STREAMS.index("p1_44k_j_192_k0")
    e = D.DecEmu(emu_so, cfgs)
    fr, ln = D.batch_arrays(fl, e.stride)
    rep0, _, _ = e.decode(fr, ln)
    e.close()
    for f in (4, 9):
        fr2 = fr.copy()
        fr2[f, s, 2] ^= 0x02
        e = D.DecEmu(emu_so, cfgs)
        rep, _, _ = e.decode(fr2, ln)
        e.close()
        st = int(rep[f, s]["status"])
        assert st & D.BAD_CRC16 and st & (D.HEADER_MISMATCH | D.OVERRUN) and not st & D.BAD_SCFCRC, hex(st)
        assert int(rep[f + 1, s]["status"]) == D.SCFCRC_UNCHECKED
        keep = np.ones(rep.shape, dtype=bool)
        keep[f:f + 2, s] = False
        assert np.array_equal(rep[keep], rep0[keep])
    assert len({int(x) for x in ln[:, s]}) == 2                  # the stream has frames of both lengths


def hostile_cases_of(fl, cfgs, stride, pad_stream):
    """every input batch of the damage, truncation, padding-bit and noise tests over the streams `fl` (`pad_stream`: one with padding
    slots, whose padding bit is flipped): [(frames, lens or None)]"""
    fr0, ln0 = D.batch_arrays(fl, stride)
    cases = [(fr0, ln0)]
    for kind, s, f, fn, _, _ in damage_cases(fl, cfgs):
        fr, ln = fr0.copy(), ln0.copy()
        b = bytearray(fr[f, s, :ln[f, s]].tobytes())
        n = fn(b)
        fr[f, s, :len(b)] = np.frombuffer(bytes(b), dtype=np.uint8)
        if n is not None:
            ln[f, s] = n
        cases.append((fr, ln))
    ln = ln0.copy(); ln[5, 2] -= 3
    cases.append((fr0, ln))
    fr = fr0.copy(); fr[4, pad_stream, 2] ^= 0x02
    cases.append((fr, ln0))
    rng = np.random.default_rng(5)
    fr = rng.integers(0, 256, (6, len(cfgs), stride), dtype=np.uint8)
    fr[1] = 0xff
    fr[2, :, :4] = [0xff, 0xfc, 0xf0, 0xff]
    ln = rng.integers(0, stride + 40, (6, len(cfgs))).astype(np.int32)
    ln[3] = -5
    cases += [(fr, ln), (fr, None)]
    return cases


def hostile_cases(goldens, stride):
    """hostile_cases_of over the damage set of the goldens"""
    fl, cfgs = _damage_set(goldens)
    return cfgs, hostile_cases_of(fl, cfgs, stride, DAMAGE_STREAMS.index("p1_44k_j_192_k0"))


def test_hostile_bytes_stay_inside_the_slot(emu_so, goldens):
    """random bytes, all-ones bytes and every length from below 0 to beyond the stride: flags, never a read outside the slot (the sanitizer
    run below is what would see one)"""
    e0 = D.DecEmu(emu_so, _damage_set(goldens)[1])
    cfgs, cases = hostile_cases(goldens, e0.stride)
    e0.close()
    for fr, ln in cases[-2:]:
        e = D.DecEmu(emu_so, cfgs)
        rep, _, pcm = e.decode(fr, ln, True, True)
        e.close()
        if ln is None:
            assert (rep["status"] & D.BAD_MASK).all()
        else:
            assert (rep["status"][ln > 0] & D.BAD_MASK).all() and (rep["status"][ln <= 0] == D.EMPTY).all()
        assert not pcm.any()


def test_damage_cases_are_clean_under_asan_ubsan(tmp_path, emu_so, goldens):
    """Item 3, second half: the same inputs -- every damage case, the truncation, the padding bit, the noise -- through the lane-loop build
    linked as a program with AddressSanitizer + UBSan (tests/emu/mp2_dec_san_main.cpp; its buffers are exactly as long as the data).  Clean,
    and the same reports, fields and PCM as the plain build, whose flags the tests above have checked."""
    exe = D.build_san_driver(tmp_path)
    e = D.DecEmu(emu_so, _damage_set(goldens)[1])
    cfgs, cases = hostile_cases(goldens, e.stride)
    got = D.run_san_driver(exe, tmp_path, cfgs, cases)
    assert len(got) == len(cases) >= 11
    for (fr, ln), g in zip(cases, got):
        e.reset()
        want = e.decode(fr, ln, True, True)
        for k in range(3):
            assert g[k].tobytes() == want[k].tobytes(), k
    e.close()


# ---- item 4: PCM ---------------------------------------------------------------------------------------------------------------------
PCM_STREAMS = ["p0_48k_s_192_k0", "p1_48k_j_128_k0", "p2_48k_d_128_k0", "p3_48k_j_128_k5", "p4_48k_s_192_k0", "p1_48k_m_64_k0",
               "p1_44k_j_192_k0", "p0_44k_m_64_k0", "p3_32k_m_64_k0", "p1_24k_d_96_k0", "p2_24k_j_64_k0", "p3_22k_j_96_k0",
               "p2_22k_m_32_k0", "p1_16k_m_32_k0", "p4_16k_d_80_k0", "p1_48k_s_192_xpad196"]


def numpy_pcm(frames, fields, cfg):
    """the numpy statement of the standard over a stream's frames (fields as the device path parsed them, checked against the taps above)"""
    nch = 1 if cfg["mode"] == "m" else 2
    syn = [D.Synth() for _ in range(nch)]
    out = np.zeros((len(frames), 2, 1152), dtype=np.int16)
    for f, fr in enumerate(frames):
        info = D.read_frame(fr, cfg)
        s = D.requantise(fields[f], info)
        for ch in range(nch):
            out[f, ch] = D.to_int16(syn[ch].frame(s[ch]))
    return out


def test_pcm_equals_the_standards_flow_chart(goldens, golden_run):
    """Item 4.  Two fp64 evaluations that differ only in summation order differ by about 1e-8 of an int16 step, so a rounding flip is rare
    but legal: |difference| <= 1 on at most 10 samples per million compared, 0 anywhere else."""
    names, gs, cfgs, frames = goldens
    _, fl, pcm, _ = golden_run
    assert len(PCM_STREAMS) >= 12
    assert {cfgs[names.index(n)]["samplerate"] for n in PCM_STREAMS} == {48000, 44100, 32000, 24000, 22050, 16000}
    assert {cfgs[names.index(n)]["mode"] for n in PCM_STREAMS} == set("sjdm") and {cfgs[names.index(n)]["psy"] for n in PCM_STREAMS} == {0, 1, 2, 3, 4}
    total = flips = 0
    for n in PCM_STREAMS:
        s = names.index(n)
        want = numpy_pcm(frames[s], fl[:, s], cfgs[s])
        got = pcm[:, s]
        d = np.abs(got.astype(np.int64) - want.astype(np.int64))
        assert d.max() <= 1, (n, int(d.max()))
        assert np.abs(want).max() > 1000, n                      # audio, not silence
        total += d.size
        flips += int((d != 0).sum())
    print(f"decode PCM vs numpy: {flips} rounding flips in {total} samples")
    assert flips * 1_000_000 <= 10 * total, (flips, total)


# ---- item 5: round trip --------------------------------------------------------------------------------------------------------------
# The analysis window weighs the newest 512 input samples, the synthesis window spreads a vector over the next 512 output samples; the two
# polyphase banks of 32 bands together are a pure delay of 512 - 32 + 1 = 481 samples (ISO/IEC 11172-3 Annex C 1.5.2: the codec's delay
# of the two filterbanks).  Decoding the encoder's output SLOTS adds the one pending frame: slot f holds frame f - 1, 1152 samples more.
FILTERBANK_DELAY = 512 - 32 + 1


def _roundtrip(emu_so, cfg, nframes=12):
    pcm = gen_pcm(11, 0, 0, nframes)
    data, _ = O.oracle_stream(pcm, samplerate=cfg["samplerate"], mode=cfg["mode"], kbps=cfg["kbps"], psy=cfg["psy"])
    # the slots of tlb_encode_* followed by the flush: slot 0 is empty (the first frame is still pending), slot f holds frame f - 1
    slots = [b""] + D.cut_frames(data, cfg)
    pcm = np.concatenate([pcm, np.zeros((1, 2, 1152), dtype=np.int16)])
    assert len(slots) == nframes + 1
    d = D.DecEmu(emu_so, [cfg])
    fr, ln = D.batch_arrays([slots], d.stride)
    rep, fl, out = d.decode(fr, ln, True, True)
    d.close()
    assert int(rep[0, 0]["status"]) == D.EMPTY and not (rep["status"][1:] & D.BAD_MASK).any()
    want = numpy_pcm(slots[1:], fl[1:, 0], cfg)                    # the numpy statement for the same frames
    assert np.abs(out[1:, 0].astype(int) - want.astype(int)).max() <= 1
    res = []
    for ch in range(2):
        x = pcm[:, ch].reshape(-1).astype(np.float64)
        y = out[:, 0, ch].reshape(-1).astype(np.float64)
        yn = np.concatenate([np.zeros(1152), want[:, ch].reshape(-1).astype(np.float64)])
        lags = np.arange(0, 4000)
        cc = np.array([np.dot(x[:len(x) - l], y[l:]) for l in lags])
        ccn = np.array([np.dot(x[:len(x) - l], yn[l:]) for l in lags])
        lag = int(lags[np.argmax(cc)])
        assert lag == int(lags[np.argmax(ccn)])
        # one clear maximum: the strict maximum over every lag tried, and there the output IS the input (correlation coefficient above
        # 0.9; a wrong lag or polarity of a broadband signal cannot reach it, a codec at these rates is far above it)
        assert (cc[lag] > np.delete(cc, lag)).all()
        a, b = x[:len(x) - lag], y[lag:]
        assert np.dot(a, b) / np.sqrt(np.dot(a, a) * np.dot(b, b)) > 0.9
        snr = 10 * np.log10(np.sum(a * a) / np.sum((a - b) ** 2))
        res.append((lag, snr))
    return res


def test_round_trip_is_audio_at_the_derived_lag(emu_so):
    """Item 5."""
    lines = []
    for cfg in (dict(samplerate=48000, mode="s", kbps=192, psy=1), dict(samplerate=24000, mode="s", kbps=96, psy=1)):
        res = _roundtrip(emu_so, cfg)
        for ch, (lag, snr) in enumerate(res):
            assert lag == 1152 + FILTERBANK_DELAY, (cfg, ch, lag)
            lines.append(f"{cfg['samplerate']} Hz '{cfg['mode']}' {cfg['kbps']} kbps psy {cfg['psy']} ch {ch}: lag {lag} samples, SNR {snr:.2f} dB")
    print("\n".join(lines))
    out = ROOT / "profiles" / "decode_roundtrip.txt"
    out.write_text("encode (oracle, pcmgen kind 0 seed 11, 12 frames) -> decode (emulation of csrc/mp2_synth.h), slots as tlb_encode_* leaves them\n"
                   "lag = one pending frame (1152) + the two filterbanks (481); SNR at that lag, information only\n" + "\n".join(lines) + "\n")


# ---- item 6: calls can be cut anywhere -----------------------------------------------------------------------------------------------
MIXED = ["p0_48k_s_128_k0", "p1_48k_j_128_k0", "p2_48k_s_192_k0", "p3_48k_j_128_k0", "p4_48k_s_128_k1", "p1_48k_m_64_k0", "p1_48k_m_64_k0",
         "p1_24k_m_64_k0", "p3_16k_s_64_k0", "p1_44k_s_128_k0", "p1_22k_m_32_k0", "p2_24k_j_64_k0", "p1_48k_j_128_xpad"]


def test_calls_can_be_cut_anywhere(emu_so, goldens):
    """Item 6: 13 mixed streams in ragged calls of 1, 7, 3, ... frames give byte-identical reports, fields and PCM to one call (with an
    empty slot in the middle of one stream); tlb_decode_reset of one stream changes no other stream's output."""
    names, gs, cfgs, frames = goldens
    idx = [names.index(n) for n in MIXED]
    cf = [cfgs[i] for i in idx]
    fls = [list(frames[i]) for i in idx]
    fls[4] = fls[4][:6] + [b""] + fls[4][6:15]                    # an empty slot: the next frame is checked against the frame before the gap
    e = D.DecEmu(emu_so, cf)
    fr, ln = D.batch_arrays(fls, e.stride)
    rep0, fl0, pcm0 = e.decode(fr, ln, True, True)
    e.close()
    assert int(rep0[6, 4]["status"]) == D.EMPTY and int(rep0[7, 4]["status"]) == 0 and not pcm0[6, 4].any()
    e = D.DecEmu(emu_so, cf)
    parts, pos = [], 0
    for n in (1, 7, 3, 2, 1, 2):
        parts.append(e.decode(fr[pos:pos + n], ln[pos:pos + n], True, True))
        pos += n
    assert pos == 16
    e.close()
    for k, whole in enumerate((rep0, fl0, pcm0)):
        assert np.array_equal(np.concatenate([p[k] for p in parts]), whole), k
    # reset of stream 3 between two calls: its next frame is a first frame (unchecked, silent history); every other stream as before
    e = D.DecEmu(emu_so, cf)
    a = e.decode(fr[:5], ln[:5], True, True)
    e.reset(3)
    b = e.decode(fr[5:], ln[5:], True, True)
    e.close()
    other = [s for s in range(len(cf)) if s != 3]
    for k, whole in enumerate((rep0, fl0, pcm0)):
        assert np.array_equal(np.concatenate([a[k], b[k]])[:, other], whole[:, other]), k
    assert int(b[0][0, 3]["status"]) == D.SCFCRC_UNCHECKED and not np.array_equal(b[2][0, 3], pcm0[5, 3])
    assert np.array_equal(b[2][1:, 3], pcm0[6:, 3])
