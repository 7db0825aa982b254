"""The threshold stage of psy models 1 and 3 after two cuts of its straight-line code (csrc/mp2_psy13.h, csrc/tl_libm.h), CPU half:
  * the subband minimum of tl_psy1_thresholds is tlm_min_rows_lt -- on the device one v_min_f64 per row, which differs from the
    reference's `if (min > LTg[j]) min = LTg[j]` only for a NaN row or for rows that are zeros of opposite sign; in the emulation it is
    that comparison, row pairs reported to TL_DBG_MINMAX (site TLM_MM_ROWS, read through emu_minmax_rows_stats);
  * the paired path of tl_psy1_stereo states its masker lists ascending in bark -- unless a kept masker lies above the threshold table's
    last line, where a line's bark value falls back to 0 -- and the device then skips tl_maskers_sorted; the emulation runs the test all
    the same and counts the channels on which it contradicts the statement (emu_order_stats).
So: emulation == oracle, SMR as raw words and frame bytes, on the 64 streams of tests/thrminlib.py; both counters read zero; the converted
site and the stated order were seen to run; and the order test that was kept still ran, on a dead-head frame among others.  The batch
runs twice: with taps (the SMR words; a tapped launch gives every mono stream a wave of its own) and without (the mono streams in pairs)."""
import ctypes

import numpy as np
import pytest

import emulib as E
import thrminlib as X


def _longs(fn, n):
    a = (ctypes.c_long * n)()
    fn(a)
    return np.array(list(a), dtype=np.int64)


def test_emulation_equals_oracle_and_both_counters_read_zero():
    S, want = X.streams(), X.oracle()
    L = E.lib()
    rows0, order0, mm0 = _longs(L.emu_minmax_rows_stats, 2), _longs(L.emu_order_stats, 4), _longs(L.emu_minmax_stats, 16)
    pcm = np.stack([p for _, _, p in S], axis=1)
    b = E.EmuBatch([cfg for _, cfg, _ in S])
    got, taps = b.encode(pcm, want_taps=True)
    tail = b.flush()
    assert b.pair_units() == 0
    b.close()
    b = E.EmuBatch([cfg for _, cfg, _ in S])
    got2, _ = b.encode(pcm)
    tail2 = b.flush()
    pairs_run = b.pair_units()
    b.close()
    rows, order, mm = _longs(L.emu_minmax_rows_stats, 2) - rows0, _longs(L.emu_order_stats, 4) - order0, _longs(L.emu_minmax_stats, 16) - mm0
    print("subband minima: unsafe row pairs %d of %d; order stated on %d channels, contradicted on %d; order tested on %d channels, %d of "
          "them dead heads; unsafe pairs at the other sites %d of %d" % (rows[0], rows[1], order[0], order[1], order[2], order[3], mm[0], mm[1]))
    for s, (name, cfg, _) in enumerate(S):
        ref, smr, nch, nsmr = want[s]
        for f in range(X.NFRAMES):
            a = np.ascontiguousarray(taps[f, s]["smr"][:nch, :nsmr]).view(np.uint64)
            assert np.array_equal(a, np.ascontiguousarray(smr[f][:nch, :nsmr]).view(np.uint64)), (name, f)
        assert got[s] + tail[s] == ref, name
        assert got2[s] + tail2[s] == ref, (name, "mono streams paired")
    assert rows[0] == 0 and rows[1] > 0                             # no NaN row, no zeros of opposite sign; and the site ran
    assert mm[0] == 0                                               # (nor at the sites of tests/test_minmax_forms_emu.py)
    assert order[1] == 0 and order[0] > 0                           # the stated order holds wherever it was stated
    # the kept test: the psy 1 channels that are not on the paired path (mono, long lists, dead heads), a dead head among them
    assert order[3] > 0 and order[2] > order[3]
    # every psy 1 channel of every frame went through the thresholds exactly once per run
    assert order[0] + order[2] == 2 * sum(want[s][2] for s, (_, cfg, _) in enumerate(S) if cfg["psy"] == 1) * X.NFRAMES
    assert pairs_run == 4 * X.NFRAMES                               # the four pairs of mono streams shared a wave each


STRESS_CONFIGS = ((48000, "s"), (44100, "j"), (32000, "s"))


@pytest.mark.parametrize("fs,mode", STRESS_CONFIGS)
def test_stated_order_is_never_contradicted_on_stress_signals(fs, mode):
    """The counter alone, on far more tone-rich frames than the byte comparison above: 64 tone-labelling stress signals (partials at the
    range boundaries and near lines 487..499, above the threshold table's last line), the comb and 16 pcmgen streams, 6 frames each.
    Wherever the paired pass vouched for the order, the order test agrees; and both answers occur."""
    from test_psy1_pairing import crafted as stress
    from test_psy1_pairing_back import comb
    from pcmgen import gen_pcm
    sig = [stress(s) for s in range(64)] + [comb(2)] + [gen_pcm(900 + k, k % 8, 0, 6) for k in range(16)]
    L = E.lib()
    o0 = _longs(L.emu_order_stats, 4)
    b = E.EmuBatch([dict(samplerate=fs, mode=mode, kbps=128, psy=1)] * len(sig))
    b.encode(np.stack(sig, axis=1))
    b.close()
    o = _longs(L.emu_order_stats, 4) - o0
    print("%d Hz '%s': order stated on %d channels, contradicted on %d; tested on %d, %d of them dead heads" % (fs, mode, o[0], o[1], o[2], o[3]))
    assert o[1] == 0
    assert o[0] > 0 and o[2] > 0 and o[0] + o[2] == 2 * 6 * len(sig)
