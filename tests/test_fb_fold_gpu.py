"""The filterbank's folded operand table on the device (csrc/mp2_fb.h): one batch per configuration of tests/fbfoldlib.py with all its
signals as streams, three frames, against the oracle: sb_sample as raw 64-bit words, scalar, bit_alloc, scfsi and the frame bytes."""
import numpy as np
import pytest

import fbfoldlib as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def M():
    import odr_audioenc_amd as mod
    mod.load_library()
    return mod


def _batch(M, cfg, n):
    return M.Batch([M.StreamConfig(samplerate=cfg["samplerate"], mode=cfg["mode"], bitrate=cfg["kbps"], psy_model=cfg["psy"])] * n)


@pytest.mark.parametrize("cfg_name", [n for n, _ in F.CONFIGS])
def test_device_equals_oracle_on_zero_sum_signals(M, cfg_name):
    cfg = dict(F.CONFIGS)[cfg_name]
    pcm = F.batch_pcm()
    b = _batch(M, cfg, pcm.shape[1])
    got, taps = b.encode(pcm, want_taps=True)
    tail = b.flush()
    b.close()
    zeros = F.check_against_oracle(cfg_name, got, tail, taps)
    print(cfg_name, "streams:", pcm.shape[1], "sb_sample words that are a zero of either sign:", zeros)
    assert zeros > 0
    # without taps: the production launch (for the mono configuration, streams share waves in pairs): the same bytes
    b = _batch(M, cfg, pcm.shape[1])
    got2, _ = b.encode(pcm)
    tail2 = b.flush()
    b.close()
    assert [g + t for g, t in zip(got2, tail2)] == [r for r, _ in F.oracle(cfg_name)]
