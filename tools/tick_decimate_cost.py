#!/usr/bin/env python3
"""What a down source adds to a tick (tlb_tick_set_down_source), and what this commit costs an object that sets none, on the GPU.

    python tools/tick_decimate_cost.py [--streams 16384] [--ticks 100] [--rounds 5] [--parent-lib PATH] [--out profiles/tick_decimate.txt]

Tick objects of 24 kHz stereo 64 kbps psy 1, egress EDI AF, in one process on one box, the legs interleaved round by round:
  parent   the library of the parent commit (--parent-lib: a libtoolame_dab_hip.so built from it), 24 kHz PCM in       } (a): `plain` against
  plain    this library, no down source, 24 kHz PCM in -- also what a host that decimates by itself sends               } `parent`
  down     this library, every stream with a 48 kHz down source: 2304 source frames per wide slot, no PCM copy-in       } (b): `down` against `plain`
Every round runs `ticks` ticks per leg with two ticks in flight (submit, submit, wait, ...) and keeps the median finished-tick interval
(host clock, wait to wait) and the median of tlb_tick_last_ms (device clock: first copy-in queued -> last copy-out done).  The file gets
the medians, minima and maxima over the rounds; the spread of a leg over its own rounds is the yardstick for (a).  A leg that cannot be
run is written as NOT MEASURED with the reason."""
import argparse
import ctypes as C
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def fmt(v):
    v = np.asarray(v, dtype=np.float64)
    return "median %.4f  min %.4f  max %.4f  (rounds: %s)" % (np.median(v), v.min(), v.max(), " ".join("%.4f" % x for x in v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=16384)
    ap.add_argument("--ticks", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "tick_decimate.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("no GPU: this tool measures, it does not estimate")
    import odr_audioenc_amd as M
    from odr_audioenc_amd import toolame as TL
    from pcmgen import gen_pcm
    ns = args.streams
    cfg = [M.StreamConfig(samplerate=24000, mode="s", bitrate=64, psy_model=1)] * ns
    nd = min(ns, 512)
    src = np.stack([np.concatenate([gen_pcm(s, 0, f, 1)[0].T.reshape(-1) for f in range(2)]) for s in range(nd)])      # [nd][4608]: 2304 source frames
    lines, objs, why = [], {}, {}
    libs = {"plain": None, "down": None}
    if args.parent_lib and Path(args.parent_lib).exists():
        libs = {"parent": TL._bind(C.CDLL(str(Path(args.parent_lib).resolve()))), **libs}
    else:
        why["parent"] = "no library of the parent commit was given (--parent-lib)"
    for name, lib in libs.items():
        t = M.Tick(cfg, egress="af", version=b"odr-audioenc_amd bench", lib=lib)
        if name == "down":
            t.set_down_source(48000)

        def fill(t=t, name=name):
            if name == "down":
                for k in range(0, ns, nd):
                    n = min(nd, ns - k)
                    np.ctypeslib.as_array((C.c_int16 * (n * 4608)).from_address(t.L.tlb_tick_down(t.h, k))).reshape(n, 4608)[:] = src[:n]
            else:
                pcm = t.pcm
                for k in range(0, ns, nd):
                    pcm[k:k + nd] = src[:min(nd, ns - k), :2304]
        for _ in range(2):                                            # both input sets, then warm-up: code objects loaded, every buffer touched
            fill(); t.run()
        for _ in range(4):
            t.run()
        objs[name] = t
    out = {k: {"interval_ms": [], "last_ms": []} for k in objs}
    for _ in range(args.rounds):
        for name, t in objs.items():
            iv, dev = np.empty(args.ticks), np.empty(args.ticks)
            t.submit()
            t0 = time.perf_counter()
            for i in range(args.ticks):
                if i + 1 < args.ticks:
                    t.submit()
                t.wait()
                t1 = time.perf_counter()
                iv[i], dev[i], t0 = (t1 - t0) * 1e3, t.last_ms(), t1
            out[name]["interval_ms"].append(float(np.median(iv[1:])))
            out[name]["last_ms"].append(float(np.median(dev)))
    for t in objs.values():
        t.close()
    lines.append("tools/tick_decimate_cost.py on %s: %d streams of 24 kHz stereo 64 kbps psy 1, EDI AF, %d ticks per round and leg with two in flight," % (torch.cuda.get_device_name(0), ns, args.ticks))
    lines.append("%d rounds interleaved in one process.  Per leg: the rounds' medians of the finished-tick interval (host clock) and of tlb_tick_last_ms (device clock)." % args.rounds)
    lines.append("A 24 kHz frame lasts 48 ms.")
    for name in ("parent", "plain", "down"):
        if name not in out:
            lines.append("%-7s NOT MEASURED: %s" % (name, why[name]))
            continue
        lines.append("%-7s finished-tick interval ms: %s" % (name, fmt(out[name]["interval_ms"])))
        lines.append("%-7s tlb_tick_last_ms         : %s" % (name, fmt(out[name]["last_ms"])))
    med = lambda n, m: float(np.median(out[n][m]))
    if "parent" in out:
        lines.append("(a) plain - parent: interval %+.4f ms, last_ms %+.4f ms; the parent's own spread over its rounds: interval %.4f ms, last_ms %.4f ms" % (
            med("plain", "interval_ms") - med("parent", "interval_ms"), med("plain", "last_ms") - med("parent", "last_ms"),
            max(out["parent"]["interval_ms"]) - min(out["parent"]["interval_ms"]), max(out["parent"]["last_ms"]) - min(out["parent"]["last_ms"])))
    else:
        lines.append("(a) plain - parent: NOT MEASURED")
    lines.append("(b) down - plain  : interval %+.4f ms, last_ms %+.4f ms (the host-side decimation the plain leg stands for is not in its figures: 147 k multiply-adds per stream and frame)" % (
        med("down", "interval_ms") - med("plain", "interval_ms"), med("down", "last_ms") - med("plain", "last_ms")))
    text = "\n".join(lines) + "\n"
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)
    print(text)


if __name__ == "__main__":
    main()
