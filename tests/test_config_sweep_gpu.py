"""Every legal Layer II configuration on the device: all 336 (sample rate, mode, bitrate) triples x psy 0-4 as ONE batch of 1680 streams
through the encoder (against the oracle, byte for byte), through the frame check / decoder (against the lane-loop emulation of the same
kernel source, bit for bit), encode -> decode without leaving the device, and one damage pass over a set with a stream of every
allocation table.  The CPU half, and what the sweep has to reach, is tests/test_config_sweep_emu.py; both share tests/sweeplib.py."""
import ctypes as C

import numpy as np
import pytest

import declib as D
import sweeplib as S
import test_decode_emu as TE
import test_decode_gpu as TG

pytestmark = pytest.mark.gpu
PSYS = (0, 1, 2, 3, 4)


@pytest.fixture(scope="module")
def M():
    import odr_audioenc_amd as mod
    mod.load_library()
    return mod


@pytest.fixture(scope="module")
def emu_so(tmp_path_factory):
    return D.build_emu(tmp_path_factory.mktemp("decemu"))


@pytest.fixture(scope="module")
def sweep():
    """-> (cfgs, pcm [6][1680][2][1152], the oracle's bytes, the oracle's taps, its frames): the five sweeps of the CPU half, side by side"""
    cfgs, pcms, data, taps = [], [], [], []
    for psy in PSYS:
        c, p = S.sweep_streams(psy)
        d, t = S.oracle_sweep(c, p)
        cfgs += c; pcms.append(p); data += d; taps += t
    assert len(cfgs) == 5 * 336 == 1680
    frames = [D.cut_frames(d, c) for d, c in zip(data, cfgs)]
    assert all(len(f) == S.NFRAMES for f in frames)
    return cfgs, np.concatenate(pcms, axis=1), data, taps, frames


def _batch(M, cfgs):
    return M.Batch([TG._mcfg(M, c) for c in cfgs])


def test_device_encoder_equals_the_oracle_on_every_configuration(M, sweep):
    """1680 streams, 6 frames in two calls, then the flush: every stream's bytes are the oracle's"""
    cfgs, pcm, data, _, _ = sweep
    b = _batch(M, cfgs)
    a, _ = b.encode(pcm[:2])
    c, _ = b.encode(pcm[2:])
    tail = b.flush()
    b.close()
    bad = [(k["samplerate"], k["mode"], k["kbps"], k["psy"]) for k, x, y, z, want in zip(cfgs, a, c, tail, data) if x + y + z != want]
    assert not bad, (len(bad), bad[:20])
    print(f"config sweep on the device, encoder: {len(cfgs)} streams x {S.NFRAMES} frames == oracle, {sum(map(len, data))} bytes")


def test_device_decoder_equals_emulation_on_every_configuration(M, emu_so, sweep):
    """the same frames through Batch.decode (tlb_decode_host) in ragged calls: reports, fields and PCM are the emulation's, bit for bit;
    no frame is bad, and the fields are the oracle's taps"""
    cfgs, _, _, taps, frames = sweep
    e = D.DecEmu(emu_so, cfgs)
    fr, ln = D.batch_arrays(frames, e.stride)
    want = e.decode(fr, ln, True, True)
    assert e.bad_frames() == 0
    e.close()
    d = TG.DevDec(M, cfgs)
    assert d.stride == fr.shape[2]
    parts, pos = [], 0
    for n in (2, 1, 3):
        parts.append(d.decode(fr[pos:pos + n], ln[pos:pos + n], True, True))
        pos += n
    assert pos == S.NFRAMES and d.bad_frames() == 0
    d.close()
    for k, name in enumerate(("report", "fields", "pcm")):
        got = np.concatenate([p[k] for p in parts])
        assert got.tobytes() == want[k].tobytes(), name
    rep = np.concatenate([p[0] for p in parts])
    fl = np.concatenate([p[1] for p in parts])
    assert (rep["status"][0] == D.SCFCRC_UNCHECKED).all() and not rep["status"][1:].any()
    cells = S.cells_of(cfgs, fl)
    assert cells == S.all_cells() and len(cells) == 87                      # the device's requantiser has been through every cell
    for s, c in enumerate(cfgs):
        for f in range(S.NFRAMES):
            S.assert_fields_equal_taps(fl[f, s], taps[s][f], 1 if c["mode"] == "m" else 2, (s, f))
    print(f"config sweep on the device, decoder: {len(cfgs)} streams x {S.NFRAMES} frames == emulation (report, fields, PCM), "
          f"{len(cells)}/87 cells, 0 bad frames")


def test_encode_then_decode_without_leaving_the_device_on_every_configuration(M, sweep):
    """tlb_encode_device_len, tlb_decode_device on the same buffers, then the flushed frame the same way: every frame of every stream is
    verified on the device (slot 0 is empty, the first frame unchecked, every later one passes with its ScF-CRC checked), zero bad frames,
    and the parsed fields are the oracle's taps"""
    cfgs, pcm, _, taps, _ = sweep
    ns, nf = len(cfgs), S.NFRAMES
    b = _batch(M, cfgs)
    H = TG.Hip()
    rsz, fsz = M.FRAME_REPORT_DTYPE.itemsize, M.FRAME_FIELDS_DTYPE.itemsize
    d_pcm, d_out, d_len = H.alloc(pcm.nbytes), H.alloc((nf + 1) * ns * b.out_stride), H.alloc((nf + 1) * ns * 4)
    d_rep, d_fl = H.alloc((nf + 1) * ns * rsz), H.alloc((nf + 1) * ns * fsz)
    H.put(d_pcm, pcm)
    assert b.L.tlb_encode_device_len(b.h, d_pcm, nf, None, None, d_out, d_len, None) == 0
    b.decode_device(d_out, d_len, nf, d_rep, d_fl)
    # the pending frame: flushed into slot nf of the same buffers, decoded as the stream's next frame
    assert b.L.tlb_flush_device_len(C.c_void_p(b.h), C.c_void_p(d_out + nf * ns * b.out_stride), C.c_void_p(d_len + nf * ns * 4), None) == 0
    b.decode_device(d_out + nf * ns * b.out_stride, d_len + nf * ns * 4, 1, d_rep + nf * ns * rsz, d_fl + nf * ns * fsz)
    assert b.decode_bad_frames() == 0
    rep = H.get(d_rep, (nf + 1, ns), M.FRAME_REPORT_DTYPE)
    fl = H.get(d_fl, (nf + 1, ns), M.FRAME_FIELDS_DTYPE)
    ln = H.get(d_len, (nf + 1, ns), np.int32)
    H.free()
    b.close()
    assert (rep["status"][0] == M.DEC_EMPTY).all() and (rep["status"][1] == M.DEC_SCFCRC_UNCHECKED).all() and not rep["status"][2:].any()
    assert (rep["crc_stored"][1:] == rep["crc_computed"][1:]).all() and (ln[0] == 0).all() and (ln[1:] > 0).all()
    for s, c in enumerate(cfgs):
        for f in range(nf):                                          # slot f + 1 holds frame f
            S.assert_fields_equal_taps(fl[f + 1, s], taps[s][f], 1 if c["mode"] == "m" else 2, (s, f))
    print(f"config sweep on the device, encode -> decode resident: {ns} streams x {nf} frames verified, 0 bad frames")


def test_device_damage_equals_emulation_on_every_table(M, emu_so):
    """the damage set of the CPU half (sweeplib.DAMAGE_CONFIGS: a stream of every allocation table) under every batch of
    test_decode_emu.hostile_cases_of: the device's reports, fields and PCM are the emulation's, byte for byte"""
    fl, cfgs = S.damage_streams()
    e = D.DecEmu(emu_so, cfgs)
    cases = TE.hostile_cases_of(fl, cfgs, e.stride, S.DAMAGE_PAD_STREAM)
    d = TG.DevDec(M, cfgs)
    assert d.stride == e.stride
    for fr, ln in cases:
        e.reset(); d.reset()
        want, got = e.decode(fr, ln, True, True), d.decode(fr, ln, True, True)
        for k in range(3):
            assert got[k].tobytes() == want[k].tobytes(), k
    assert d.bad_frames() == e.bad_frames() >= 6 * len(cfgs)                # (the batch of noise without lengths alone: every frame of it)
    e.close(); d.close()
