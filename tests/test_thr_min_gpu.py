"""The device half of tests/test_thr_min_emu.py: the streams of tests/thrminlib.py through Batch.encode_device, bytes against the oracle.
What the emulation cannot see shows here: a v_min_f64 over a subband's rows that returned another row than the reference's comparison, or
a masker span bisected over a list that was not ascending after all (the paired path of tl_psy1_stereo does not test the order on the
device) -- either would change an SMR value, and with it the allocation and the bytes of these frames."""
import numpy as np
import pytest

import test_decode_gpu as TG
import thrminlib as X

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def M():
    import odr_audioenc_amd as mod
    mod.load_library()
    return mod


def _device_bytes(M, cfgs, pcm):
    """pcm [nframes, nstreams, 2, 1152] -> per stream the bytes of every frame and the flushed one"""
    nf, ns = pcm.shape[:2]
    b = M.Batch([M.StreamConfig(samplerate=c["samplerate"], mode=c["mode"], bitrate=c["kbps"], psy_model=c["psy"]) for c in cfgs])
    H = TG.Hip()
    d_pcm, d_out = H.alloc(pcm.nbytes), H.alloc(nf * ns * b.out_stride)
    H.put(d_pcm, pcm)
    b.encode_device(d_pcm, nf, d_out)
    out = H.get(d_out, (nf, ns, b.out_stride), np.uint8)
    tail = b.flush()
    H.free()
    b.close()
    # slot 0 of a batch's first call is empty (one frame of latency); a later slot holds frame_bytes, one more with the header's padding bit
    return [b"".join(out[f, s, : b.frame_bytes[s] + ((int(out[f, s, 2]) >> 1) & 1)].tobytes() for f in range(1, nf)) + tail[s] for s in range(ns)]


def test_mixed_batch_equals_oracle(M):
    """64 streams x 2 frames in one batch: psy 1 and 3; 's', 'j' and mono pairs; 48, 44.1 and 32 kHz; dead heads and long tone lists"""
    S, want = X.streams(), X.oracle()
    got = _device_bytes(M, [cfg for _, cfg, _ in S], np.ascontiguousarray(np.stack([p for _, _, p in S], axis=1)))
    bad = [name for s, (name, _, _) in enumerate(S) if got[s] != want[s][0]]
    assert not bad, bad


def test_flagship_shape_equals_oracle(M):
    """8 streams x 4 frames of the benchmark's flagship configuration (48 kHz, 's', 128 kbps, psy 1: tl_frame_kernel<1, false, 2>)"""
    cfg, pcm, want = X.flagship()
    got = _device_bytes(M, [cfg] * pcm.shape[1], pcm)
    bad = [s for s in range(pcm.shape[1]) if got[s] != want[s]]
    assert not bad, bad
