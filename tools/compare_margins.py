#!/usr/bin/env python3
"""Where the compare monitor's default correlation ratio comes from (TLB_COMPARE_DEFAULT_*), measured on the CPU emulation.

    python tools/compare_margins.py [--frames 6] [--jobs 8] [--out profiles/compare_margins.txt]

For every (rate, mode, bitrate) of the configuration sweep (tests/sweeplib.py legal_configs, 336) with psy model 1, three streams are
encoded by the encoder emulation and decoded by the decode emulation: the programme-like signals of tests/pcmgen.py (kind 0 tones + noise,
kind 7 the same under a stepped envelope, kind 0 again) with independent seeds, the same three programmes for every configuration.  Per configuration the file records
  healthy_min   the smallest correlation sxy / sqrt(sxx syy) over the judged channels (sxx >= the default min_energy) of every stream
                against its OWN input at the delay, slots with a whole frame of history
  mispaired_max the largest over stream k's decode against stream k + 1's input, same slots and channels
A default between the largest mispaired_max and the smallest healthy_min separates the two everywhere.  Three programmes and a few frames
are a small sample, so a configuration counts as "compare not meaningful with default params" when either figure comes within MARGIN
(0.05) of the chosen ratio; those are listed at the end, and after them the ones within 0.1, which are close but counted as usable."""
import argparse
import sys
from concurrent.futures import ProcessPoolExecutor
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
KINDS = (0, 7, 0)
MIN_ENERGY, NUM, DEN = 1152 * 256 * 256, 3, 8
MARGIN = 0.05


def one(args):
    triple, nframes, dec_so = args
    import comparelib as CL
    import declib as D
    import emulib as E
    from pcmgen import gen_pcm
    fs, mode, kbps = triple
    cfg = dict(samplerate=fs, mode=mode, kbps=kbps, psy=1)
    ns, nch = len(KINDS), 1 if mode == "m" else 2
    pcm = np.stack([gen_pcm(seed=4000 + 131 * s, kind=k, frame=0, nframes=nframes) for s, k in enumerate(KINDS)], axis=1)
    e = E.EmuBatch([cfg] * ns)
    out = np.zeros((nframes, ns, e.stride), dtype=np.uint8)
    lens = np.zeros((nframes, ns), dtype=np.int32)
    e.L.emu_encode_len(e.h, pcm.ctypes.data, nframes, None, None, out.ctypes.data, e.stride, None, lens.ctypes.data)
    e.close()
    d = D.DecEmu(dec_so, [cfg] * ns)
    rep, _, dec = d.decode(out, lens, False, True)
    d.close()
    assert not (rep["status"][1:] & (D.EMPTY | D.BAD_MASK)).any(), triple
    healthy, mis = [], []
    for s in range(ns):
        for c in range(nch):
            x = pcm[:, s, c].reshape(-1).astype(np.int64)
            z = pcm[:, (s + 1) % ns, c].reshape(-1).astype(np.int64)
            for f in range(2, nframes):
                lo, hi = (f - 1) * 1152 - CL.DELAY, f * 1152 - CL.DELAY
                y = dec[f, s, c].astype(np.int64)
                for src, dst in ((x, healthy), (z, mis)):
                    sxx, syy, sxy = int((src[lo:hi] ** 2).sum()), int((y * y).sum()), int((src[lo:hi] * y).sum())
                    if sxx >= MIN_ENERGY:
                        dst.append(CL.corr(sxy, sxx, syy))
    return triple, min(healthy), max(mis), len(healthy)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=6)
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "compare_margins.txt"))
    a = ap.parse_args()
    import declib as D
    import emulib as E
    import sweeplib as SW
    import tempfile
    E.lib()                                                          # built once, before the workers load it
    with tempfile.TemporaryDirectory() as td:
        so = D.build_emu(td)
        with ProcessPoolExecutor(a.jobs) as ex:
            rows = list(ex.map(one, [(t, a.frames, so) for t in SW.legal_configs()], chunksize=4))
    thr = NUM / DEN
    touch = [r for r in rows if r[1] < thr + MARGIN or r[2] > thr - MARGIN]
    near = [r for r in rows if r not in touch and (r[1] < thr + 0.1 or r[2] > thr - 0.1)]
    rest = [r for r in rows if r not in touch]
    lines = ["# compare monitor: correlation of decoded against input audio, CPU emulation (tools/compare_margins.py)",
             "# psy 1, signals pcmgen kinds %s with independent seeds, %d frames, judged channels only (sxx >= %d), delay 481" % (KINDS, a.frames, MIN_ENERGY),
             "# rate mode kbps  healthy_min  mispaired_max  judged"]
    lines += ["%5d %s %3d  %.4f  %+.4f  %d" % (t[0], t[1], t[2], h, m, n) for t, h, m, n in rows]
    lines += ["# over all %d configurations: healthy_min %.4f, mispaired_max %+.4f; default ratio %d/%d = %.3f" % (len(rows), min(r[1] for r in rows), max(r[2] for r in rows), NUM, DEN, thr),
              "# compare not meaningful with default params (healthy_min < %.3f or mispaired_max > %.3f, i.e. within %.2f of the ratio): %d configuration(s)" % (thr + MARGIN, thr - MARGIN, MARGIN, len(touch))]
    lines += ["#   %d %s %d  healthy_min %.4f  mispaired_max %+.4f" % (t[0], t[1], t[2], h, m) for t, h, m, n in touch]
    lines += ["# over the other %d: healthy_min %.4f, mispaired_max %+.4f" % (len(rest), min(r[1] for r in rest), max(r[2] for r in rest)),
              "# of those, within 0.1 of the ratio (usable, with little room): %d configuration(s)" % len(near)]
    lines += ["#   %d %s %d  healthy_min %.4f  mispaired_max %+.4f" % (t[0], t[1], t[2], h, m) for t, h, m, n in near]
    Path(a.out).write_text("\n".join(lines) + "\n")
    print("\n".join(lines[3 + len(rows):]))


if __name__ == "__main__":
    main()
