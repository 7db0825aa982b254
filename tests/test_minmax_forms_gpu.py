"""The device half of tests/test_minmax_forms_emu.py: the same groups of streams (tests/minmaxlib.py) through Batch.encode_device, bytes
against the oracle.  The emulation cannot see a deviation of the one-instruction maxima and minima (csrc/tl_libm.h: in the emulation the
helpers are the statements they replace); a v_max_f64 / v_min_f64 that returned another operand than the comparison would show here, in
the scalefactors, the tone candidates, the masker spans or the SMR of these frames."""
import numpy as np
import pytest

import minmaxlib as X
import test_decode_gpu as TG

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def M():
    import odr_audioenc_amd as mod
    mod.load_library()
    return mod


@pytest.mark.parametrize("gi", range(len(X.groups())), ids=[g[0] for g in X.groups()])
def test_device_equals_oracle(M, gi):
    name, cfg, pcms = X.groups()[gi]
    want = X.oracle_bytes(gi)
    ns, nf = len(pcms), X.NFRAMES
    pcm = np.stack(pcms, axis=1)
    b = M.Batch([M.StreamConfig(samplerate=cfg["samplerate"], mode=cfg["mode"], bitrate=cfg["kbps"], psy_model=cfg["psy"])] * ns)
    H = TG.Hip()
    d_pcm, d_out = H.alloc(pcm.nbytes), H.alloc(nf * ns * b.out_stride)
    H.put(d_pcm, pcm)
    b.encode_device(d_pcm, nf, d_out)
    out = H.get(d_out, (nf, ns, b.out_stride), np.uint8)
    tail = b.flush()
    H.free()
    b.close()
    for s in range(ns):
        # slot 0 of a batch's first call is empty (one frame of latency); a later slot holds frame_bytes, one more with the header's padding bit
        got = b"".join(out[f, s, : b.frame_bytes[s] + ((int(out[f, s, 2]) >> 1) & 1)].tobytes() for f in range(1, nf)) + tail[s]
        assert got == want[s], (name, s)
