"""Frame check and decode on the device (tlb_decode_*): byte for byte against the lane-loop emulation of the same kernel source on every
golden and on the damage cases, encode -> decode without leaving the device, the full population verified frame by frame, and the
example's --verify switch."""
import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import declib as D
import oraclelib as O
import test_decode_emu as TE
from pcmgen import gen_pcm

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def M():
    import odr_audioenc_amd as mod
    mod.load_library()
    return mod


@pytest.fixture(scope="module")
def emu_so(tmp_path_factory):
    return D.build_emu(tmp_path_factory.mktemp("decemu"))


@pytest.fixture(scope="module")
def goldens():
    names = D.golden_names()
    assert len(names) == 126
    gs = [np.load(D.GOLDEN / (n + ".npz")) for n in names]
    cfgs = [D.golden_cfg(g) for g in gs]
    return names, gs, cfgs, [D.cut_frames(g["data"], c) for g, c in zip(gs, cfgs)]


def _mcfg(M, c):
    return M.StreamConfig(samplerate=c["samplerate"], mode=c["mode"], bitrate=c["kbps"], psy_model=c["psy"], pad_len=c["pad_len"])


class DevDec:
    """the device path with the interface of declib.DecEmu"""

    def __init__(self, M, cfgs):
        self.b = M.Batch([_mcfg(M, c) for c in cfgs])
        self.stride = self.b.out_stride

    def decode(self, frames, lens, want_fields=True, want_pcm=False):
        return self.b.decode(frames, lens, want_fields, want_pcm)

    def reset(self, s=-1):
        self.b.decode_reset(s)

    def bad_frames(self):
        return self.b.decode_bad_frames()

    def close(self):
        self.b.close()


def test_device_equals_emulation_on_every_golden(M, emu_so, goldens):
    """Item 7: reports, fields and PCM of all 126 goldens in ONE mixed batch, in ragged calls on the device against one call of the emulation."""
    names, gs, cfgs, frames = goldens
    e = D.DecEmu(emu_so, cfgs)
    fr, ln = D.batch_arrays(frames, e.stride)
    want = e.decode(fr, ln, True, True)
    e.close()
    d = DevDec(M, cfgs)
    assert d.stride == fr.shape[2]
    parts, pos = [], 0
    for n in (5, 1, 10):
        parts.append(d.decode(fr[pos:pos + n], ln[pos:pos + n], True, True))
        pos += n
    assert d.bad_frames() == 0
    d.close()
    for k, name in enumerate(("report", "fields", "pcm")):
        got = np.concatenate([p[k] for p in parts])
        assert got.tobytes() == want[k].tobytes(), name
    assert (want[0]["status"][0] == D.SCFCRC_UNCHECKED).all() and not want[0]["status"][1:].any()


def test_device_finds_and_contains_damage(M, goldens):
    """Item 7, second half: the damage cases of tests/test_decode_emu.py on the device."""
    fl, cfgs = TE._damage_set(goldens)
    TE.run_damage(lambda c: DevDec(M, c), fl, cfgs)


def test_device_damage_equals_emulation(M, emu_so, goldens):
    """every input batch of the damage, truncation, padding-bit and noise tests (tests/test_decode_emu.py hostile_cases): the device's reports,
    fields and PCM are the emulation's, byte for byte"""
    e = D.DecEmu(emu_so, TE._damage_set(goldens)[1])
    cfgs, cases = TE.hostile_cases(goldens, e.stride)
    d = DevDec(M, cfgs)
    for fr, ln in cases:
        e.reset(); d.reset()
        want, got = e.decode(fr, ln, True, True), d.decode(fr, ln, True, True)
        for k in range(3):
            assert got[k].tobytes() == want[k].tobytes(), k
    assert d.bad_frames() == e.bad_frames() > 100
    e.close(); d.close()


class Hip:
    """device buffers through the HIP runtime the library itself has loaded (found in this process's map): hipMalloc / hipMemcpy / hipFree"""

    def __init__(self):
        path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
        self.L = C.CDLL(path)
        self.L.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.L.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
        self.L.hipFree.argtypes = [C.c_void_p]
        self.bufs = []

    def alloc(self, nbytes):
        p = C.c_void_p()
        assert self.L.hipMalloc(C.byref(p), nbytes) == 0 and self.L.hipMemset(p, 0, nbytes) == 0
        self.bufs.append(p)
        return p.value

    def put(self, ptr, arr):
        arr = np.ascontiguousarray(arr)
        assert self.L.hipMemcpy(ptr, arr.ctypes.data, arr.nbytes, 1) == 0

    def get(self, ptr, shape, dtype):
        out = np.zeros(shape, dtype=dtype)
        assert self.L.hipDeviceSynchronize() == 0 and self.L.hipMemcpy(out.ctypes.data, ptr, out.nbytes, 2) == 0
        return out

    def free(self):
        for p in self.bufs:
            self.L.hipFree(p)
        self.bufs = []


def _taps_equal(fields, taps, nch=2):
    ba = fields["bit_alloc"].astype(int)
    assert np.array_equal(ba[:nch], taps["bit_alloc"][:nch])
    m = ba != 0
    assert np.array_equal(fields["scfsi"][m], taps["scfsi"][m])
    assert np.array_equal(fields["scalar"][np.broadcast_to(m[:, None, :], (2, 3, 32))], taps["scalar"][np.broadcast_to(m[:, None, :], (2, 3, 32))])
    own = m.copy()
    own[1, taps["jsbound"]:] = False
    ms = np.broadcast_to(own[:, None, None, :], (2, 3, 12, 32))
    assert ms.any() and np.array_equal(fields["subband"][ms].astype(np.int64), taps["subband"][ms].astype(np.int64))


def test_encode_then_decode_without_leaving_the_device(M):
    """Item 8: 4096 streams x 32 frames of configs[1] (48 kHz 's' 128 kbps psy 1): tlb_encode_device_len, then tlb_decode_device on the same
    buffers.  Zero BAD_* flags, tlb_decode_bad_frames == 0, slot 0 EMPTY, fields of three sampled streams equal the oracle's taps."""
    ns, nf, nbase = 4096, 32, 64
    base = np.stack([gen_pcm(s, 0, 0, nf) for s in range(nbase)], axis=1)
    pcm = np.tile(base, (1, ns // nbase, 1, 1))
    b = M.Batch([M.StreamConfig(mode="s", psy_model=1)] * ns)
    H = Hip()
    d_pcm, d_out, d_len = H.alloc(pcm.nbytes), H.alloc(nf * ns * b.out_stride), H.alloc(nf * ns * 4)
    d_rep, d_fl = H.alloc(nf * ns * M.FRAME_REPORT_DTYPE.itemsize), H.alloc(nf * ns * M.FRAME_FIELDS_DTYPE.itemsize)
    d_dec = H.alloc(pcm.nbytes)
    H.put(d_pcm, pcm)
    assert b.L.tlb_encode_device_len(b.h, d_pcm, nf, None, None, d_out, d_len, None) == 0
    b.decode_device(d_out, d_len, nf, d_rep, d_fl, d_dec)
    assert b.decode_bad_frames() == 0
    rep = H.get(d_rep, (nf, ns), M.FRAME_REPORT_DTYPE)
    assert (rep["status"][0] == M.DEC_EMPTY).all() and (rep["status"][1] == M.DEC_SCFCRC_UNCHECKED).all() and not rep["status"][2:].any()
    assert (rep["crc_stored"] == rep["crc_computed"]).all()
    fl = H.get(d_fl, (nf, ns), M.FRAME_FIELDS_DTYPE)
    dec = H.get(d_dec, (nf, ns, 2, 1152), np.int16)
    assert np.array_equal(dec[:, nbase:2 * nbase], dec[:, :nbase]) and np.abs(dec[2:].astype(int)).max() > 1000
    for s in (0, 17, 4095):
        e = O.OracleEncoder(mode="s", kbps=128, psy=1)
        for f in range(nf - 1):
            e.encode(pcm[f, s])
            _taps_equal(fl[f + 1, s], e.taps())                      # slot f + 1 holds frame f
        e.close()
    H.free()
    b.close()


def test_full_population_every_frame_verified_on_the_device(M):
    """Item 9: 131 072 psy-3 streams x 1 frame x 4 launches; every frame of every launch is checked on the device (CRC-16, ScF-CRC against
    the frame of the launch before, header, bit budget) -- the check tests/test_hip_parity.py can only sample."""
    ns, nbase, launches = 131072, 128, 4
    b = M.Batch([M.StreamConfig(mode="s", psy_model=3)] * ns)
    H = Hip()
    d_pcm, d_out, d_len = H.alloc(ns * 4608), H.alloc(ns * b.out_stride), H.alloc(ns * 4)
    d_rep = H.alloc(ns * M.FRAME_REPORT_DTYPE.itemsize)
    for k in range(launches):
        base = np.stack([gen_pcm(s, 0, k, 1) for s in range(nbase)], axis=1)
        H.put(d_pcm, np.tile(base, (1, ns // nbase, 1, 1)))
        assert b.L.tlb_encode_device_len(b.h, d_pcm, 1, None, None, d_out, d_len, None) == 0
        b.decode_device(d_out, d_len, 1, d_rep)
        st = H.get(d_rep, (ns,), M.FRAME_REPORT_DTYPE)["status"]
        assert (st == (M.DEC_EMPTY, M.DEC_SCFCRC_UNCHECKED, 0, 0)[k]).all(), (k, np.unique(st))
    assert b.decode_bad_frames() == 0
    H.free()
    b.close()


def test_argument_errors_change_nothing(M):
    b = M.Batch([M.StreamConfig()])
    L = b.L
    rep = np.zeros(1, dtype=M.FRAME_REPORT_DTYPE)
    fr = np.zeros((1, 1, b.out_stride), dtype=np.uint8)
    assert L.tlb_decode_host(None, fr.ctypes.data, None, 1, rep.ctypes.data, None, None) == 18
    assert L.tlb_decode_host(b.h, None, None, 1, rep.ctypes.data, None, None) == 18
    assert L.tlb_decode_host(b.h, fr.ctypes.data, None, 0, rep.ctypes.data, None, None) == 18
    assert L.tlb_decode_host(b.h, fr.ctypes.data, None, 1, None, None, None) == 18
    assert L.tlb_decode_device(b.h, 0x1001, None, 1, 0x2000, None, None, None) == 18                        # a misaligned device pointer: refused before any use
    assert L.tlb_decode_reset(b.h, 1) == 18 and L.tlb_decode_reset(b.h, -2) == 18 and L.tlb_decode_reset(b.h, -1) == 0
    assert b.decode_bad_frames() == 0
    b.close()


def test_example_verify_switch(tmp_path):
    """Item 10: examples/mp2enc --verify decodes what it just encoded and exits 0; with the example's test-only environment hook
    MP2ENC_TEST_CORRUPT (a byte offset into its frame buffer, flipped before the check) it exits non-zero."""
    from test_example_mp2enc import build
    exe = build(tmp_path)
    g = np.load(D.GOLDEN / "p1_48k_j_128_k0.npz")
    c = D.golden_cfg(g)
    pcm = gen_pcm(c["seed"], c["kind"], 0, c["nframes"])                # a golden's PCM, interleaved s16le
    (tmp_path / "in.pcm").write_bytes(pcm.transpose(0, 2, 1).reshape(-1).astype("<i2").tobytes())
    cmd = [str(exe), str(tmp_path / "in.pcm"), str(tmp_path / "out.mp2"), "-m", "j", "-b", "128", "-p", "1", "-n", "3", "--verify"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "verify ok: 48 frames" in r.stderr, r.stdout + r.stderr
    assert (tmp_path / "out.mp2").read_bytes() == bytes(g["data"])
    stride = 384
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(os.environ, MP2ENC_TEST_CORRUPT=str(5 * 3 * stride + 10)))
    assert r.returncode == 3 and "verify failed" in r.stderr, r.stdout + r.stderr
