"""The quantiser's re-deal (csrc/mp2_pack.h K6, csrc/mp2_wave.h TL_Q_REDEAL): frames with at most TL_Q_REDEAL_MAX = 48 live cells
(bit_alloc != 0) pass their samples through LDS a granule at a time and quantise one triple per lane; the others, frames with
joint-coded subbands, frames with taps and mono pairs keep the lane-per-cell loop.  Kernel source through the lane-loop emulation
against the oracle, byte for byte, with the emulation's own count of which way every frame went (emu_redeal_stats).  CPU only.

Live cells are steered by the bitrate (48 kHz 's': sblimit 8 at 64 kbps, 27 above), by silence in one channel and by noise cut off
above a subband.  The mix is built so that the 's' frames cover: n <= 16, 17..32 and 33..48 (three, six and nine rounds instead of
twelve), n <= 21, n = 32, n = 33, n = 48 (the threshold) and n = 54 (every cell live: above it, lane-per-cell loop)."""
import ctypes

import numpy as np
import pytest

import emulib as E
import oraclelib as O
from pcmgen import gen_pcm

REDEAL_MAX = 48


def _stats():
    L = E.lib()
    a = (ctypes.c_long * 132)()
    L.emu_redeal_stats(a)
    return np.array(list(a), dtype=np.int64)


def _band_noise(seed, k0, k1, nframes, amp=8000):
    """Gaussian noise cut off just below subband k of each channel (750 Hz per subband at 48 kHz); k = 0: a silent channel."""
    rng = np.random.default_rng(seed)
    n = nframes * 1152
    out = np.zeros((2, n))
    for ch, k in enumerate((k0, k1)):
        if k == 0:
            continue
        X = np.fft.rfft(rng.standard_normal(n))
        X[np.arange(X.size) * 48000.0 / n >= 750.0 * k - 60] = 0
        y = np.fft.irfft(X, n)
        out[ch] = y / np.abs(y).max() * amp
    return np.ascontiguousarray(np.rint(out).astype(np.int16).reshape(2, nframes, 1152).transpose(1, 0, 2))


def _run(pcms, want_taps=False, **cfg):
    """streams of one configuration in one batch -> (all equal the oracle, frames [old, new], histograms of n [old, new], taps)"""
    b = E.EmuBatch([cfg] * len(pcms))
    s0 = _stats()
    got, taps = b.encode(np.stack(pcms, axis=1), want_taps=want_taps)
    tail = b.flush()
    pairs = b.pair_units()
    b.close()
    d = _stats() - s0
    for s, pcm in enumerate(pcms):
        ref, _ = O.oracle_stream(pcm, samplerate=cfg.get("samplerate", 48000), mode=cfg["mode"], kbps=cfg["kbps"], psy=cfg["psy"])
        assert got[s] + tail[s] == ref, (cfg, s)
    return d[:2], (d[2:67], d[67:132]), taps, pairs


# (kbps, name, pcm) of the 's' cases; 6 frames each, 3 for the one that is meant to stay on the lane-per-cell loop
def _s_cases():
    nf = 6
    return [
        (64, "tones+noise", gen_pcm(77, 0, 0, nf)), (64, "full-scale noise", gen_pcm(81, 4, 0, nf)),
        (128, "tones+noise", gen_pcm(77, 0, 0, nf)), (128, "full-scale noise", gen_pcm(81, 4, 0, nf)),
        (128, "one channel silent", _band_noise(5, 27, 0, nf)), (128, "noise below subband 24", _band_noise(5, 24, 24, nf)),
        (192, "tones+noise", gen_pcm(77, 0, 0, nf)), (192, "+-1 LSB noise", gen_pcm(83, 6, 0, nf)),
        (192, "noise below subband 16", _band_noise(5, 16, 16, nf)), (192, "noise below subbands 17 / 16", _band_noise(5, 17, 16, nf)),
        (384, "+-1 LSB noise", gen_pcm(83, 6, 0, nf)), (384, "tones+noise", gen_pcm(77, 0, 0, 3)),
        (384, "stepped envelope", gen_pcm(84, 7, 0, nf)),
    ]


def test_redeal_s_streams_cover_the_live_cell_counts():
    went = np.zeros(2, dtype=np.int64)
    hist = [np.zeros(65, dtype=np.int64), np.zeros(65, dtype=np.int64)]
    for kbps, name, pcm in _s_cases():
        w, h, _, _ = _run([pcm], mode="s", kbps=kbps, psy=1)
        print(kbps, name, "lane-per-cell / re-dealt frames:", w.tolist(),
              "live cells (re-dealt):", {int(n): int(c) for n, c in enumerate(h[1]) if c}, "(lane-per-cell):", {int(n): int(c) for n, c in enumerate(h[0]) if c})
        assert w.sum() == pcm.shape[0]
        assert h[1][REDEAL_MAX + 1:].sum() == 0 and h[0][:REDEAL_MAX + 1].sum() == 0, "the dispatch is by the live-cell count alone"
        went += w
        hist[0] += h[0]
        hist[1] += h[1]
    old, new = hist
    print("frames lane-per-cell / re-dealt:", went.tolist())
    assert went[1] >= 0.9 * went.sum()
    assert new[1:17].sum() > 0 and new[17:33].sum() > 0 and new[33:49].sum() > 0       # three, six and nine rounds
    assert new[1:22].sum() > 0                                                         # three lanes or more per cell
    assert new[32] > 0 and new[33] > 0                                                 # either side of a whole round of 16 cells
    assert new[REDEAL_MAX] > 0 and old[54] > 0 and old[49:].sum() == went[0]           # the threshold itself and its other side


def test_redeal_sees_grouped_and_ungrouped_classes():
    """The same frames with taps (which keep the lane-per-cell loop, and equal the oracle too) show what the re-dealt frames carried:
    bit_alloc 1 is the grouped 3-step class in every allocation table, 2 on subbands 3.. the 5-step class, 4 on subbands 3..10 the 9-step
    class, and 5 and above are ungrouped classes (ISO 11172-3 Table B.2a)."""
    pcm = gen_pcm(77, 0, 0, 6)
    w, _, taps, _ = _run([pcm], want_taps=True, mode="s", kbps=128, psy=1)
    assert w[1] == 0 and w[0] == 6
    ba = taps[:, 0]["bit_alloc"]                                       # [frame][ch][sb]
    assert (ba == 1).any() and (ba[:, :, 3:] == 2).any() and (ba[:, :, 3:11] == 4).any() and (ba >= 5).any()
    w, h, _, _ = _run([pcm], mode="s", kbps=128, psy=1)
    assert w[1] == 6 and w[0] == 0
    assert int((h[1] * np.arange(65)).sum()) == int((ba != 0).sum())       # the same live cells, frame for frame in total


@pytest.mark.parametrize("psy", (0, 2, 3))
def test_redeal_other_models_share_the_encoder(psy):
    w, _, _, _ = _run([gen_pcm(90 + psy, 0, 0, 4), gen_pcm(91 + psy, 7, 0, 4)], mode="s", kbps=128, psy=psy)
    assert w[1] > 0 and w.sum() == 8


def test_joint_frames_and_mono_pairs_keep_the_lane_per_cell_loop():
    pcm = gen_pcm(3, 0, 0, 6)
    w, _, _, _ = _run([pcm], mode="j", kbps=128, psy=1)              # 128 kbps 'j' on this signal: joint-coded subbands in every frame
    assert w[1] == 0 and w[0] == 6
    # two mono streams of one configuration share a wave (tl_encode_pair): not a frame of tl_encode_frame at all
    w, _, _, pairs = _run([gen_pcm(3, 0, 0, 6), gen_pcm(4, 0, 0, 6)], mode="m", kbps=64, psy=1)
    assert pairs == 6 and w.sum() == 0
    # a lone mono stream is a frame of tl_encode_frame with every second lane idle: re-dealt
    w, _, _, pairs = _run([gen_pcm(3, 0, 0, 6)], mode="m", kbps=64, psy=1)
    assert pairs == 0 and w[1] == 6
