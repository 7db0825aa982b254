#!/usr/bin/env python3
"""What a down feed costs and saves per tick (tlb_tick_set_down_feed), and what this commit costs an object that sets none, on the GPU.

    python tools/tick_feed_down_cost.py [--streams 16384] [--ticks 100] [--rounds 5] [--psy 3] [--parent-lib PATH] [--parent-legs] [--out profiles/tick_feed_down.txt]

Tick objects of 24 kHz stereo 64 kbps, egress EDI AF, in one process on one box, the legs interleaved round by round:
  parent   the library of the parent commit (--parent-lib: a libtoolame_dab_hip.so built from it), 24 kHz PCM in       } (a): `plain` against
  plain    this library, no down feed, 24 kHz PCM in                                                                    } `parent`
  fed      this library, every stream with a 48 kHz 192 kbps down feed: two frames of 576 bytes and two lengths per     } (b): `fed` against
           stream and tick over the link (1160 bytes), no PCM copy-in                                                   } `down`
  down     this library, the same audio as wide PCM through set_down_source(48000): 9216 bytes per stream and tick
Every round runs `ticks` ticks per leg with two ticks in flight (submit, submit, wait, ...) and keeps the median finished-tick interval
(host clock, wait to wait) and the median of tlb_tick_last_ms (device clock: first copy-in queued -> last copy-out done).  The file gets
the medians, minima and maxima over the rounds; the spread of the parent leg over its own rounds is the yardstick for (a).  A leg that
cannot be run is written as NOT MEASURED with the reason.
--parent-legs (a parent commit that has both families): the `fed` and `down` legs run on the parent's library too (`p-fed`, `p-down`), and
every leg of this library is set against the same leg of the parent's, (c): the difference of the medians next to the spread (max - min over
the rounds) the parent's leg shows in the same run, on both clocks."""
import argparse
import ctypes as C
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
LEGS = ("parent", "plain", "fed", "down", "p-fed", "p-down")
PARENT_OF = {"plain": "parent", "fed": "p-fed", "down": "p-down"}


def fmt(v):
    v = np.asarray(v, dtype=np.float64)
    return "median %.4f  min %.4f  max %.4f  (rounds: %s)" % (np.median(v), v.min(), v.max(), " ".join("%.4f" % x for x in v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=16384)
    ap.add_argument("--ticks", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--psy", type=int, default=3)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--parent-legs", action="store_true", help="run the fed and down legs on --parent-lib too and compare leg by leg")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "tick_feed_down.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("no GPU: this tool measures, it does not estimate")
    import odr_audioenc_amd as M
    from odr_audioenc_amd import toolame as TL
    import declib as D
    from pcmgen import gen_pcm
    ns = args.streams
    cfg = [M.StreamConfig(samplerate=24000, mode="s", bitrate=64, psy_model=args.psy)] * ns
    nd = min(ns, 512)
    src = np.stack([np.concatenate([gen_pcm(s, 0, f, 1)[0].T.reshape(-1) for f in range(2)]) for s in range(nd)])      # [nd][4608]: 2304 source frames
    # two consecutive 48 kHz 192 kbps frames of one programme: every stream's two slots of every tick
    e = M.Batch([M.StreamConfig(samplerate=48000, mode="s", bitrate=192, psy_model=1)])
    data, _ = e.encode(gen_pcm(7, 0, 0, 4)[:, None])
    e.close()
    pair = D.cut_frames(data[0], dict(samplerate=48000, kbps=192))[1:3]
    assert len(pair) == 2 and all(len(f) == 576 for f in pair)
    fc = M.FeedConfig(samplerate=48000, bitrate=192, channels=2)
    lines, objs, why = [], {}, {}
    libs = {"plain": None, "fed": None, "down": None}
    if args.parent_lib and Path(args.parent_lib).exists():
        parent = TL._bind(C.CDLL(str(Path(args.parent_lib).resolve())))
        libs = {"parent": parent, **libs, **({"p-fed": parent, "p-down": parent} if args.parent_legs else {})}
    else:
        why["parent"] = "no library of the parent commit was given (--parent-lib)"
    for leg, lib in libs.items():
        name = leg[2:] if leg.startswith("p-") else leg               # what the leg does, whichever library does it
        t = M.Tick(cfg, egress="af", version=b"odr-audioenc_amd bench", lib=lib)
        if name == "down":
            t.set_down_source(48000)
        if name == "fed":
            t.set_down_feed(-1, fc)

        def fill(t=t, name=name):
            if name == "down":
                for k in range(0, ns, nd):
                    n = min(nd, ns - k)
                    np.ctypeslib.as_array((C.c_int16 * (n * 4608)).from_address(t.L.tlb_tick_down(t.h, k))).reshape(n, 4608)[:] = src[:n]
            elif name == "fed":
                fr = t.down_feed
                for j in range(2):
                    fr[:, j, :576] = np.frombuffer(pair[j], dtype=np.uint8)
            else:
                pcm = t.pcm
                for k in range(0, ns, nd):
                    pcm[k:k + nd] = src[:min(nd, ns - k), :2304]

        def submit(t=t, name=name):
            if name == "fed":
                t.down_feed_len[:] = 576                              # (a set of lengths comes back all 0; the frames stay where they were put)
            t.submit()
        for _ in range(2):                                            # both input sets, then warm-up: code objects loaded, every buffer touched
            fill(); submit(); t.wait()
        for _ in range(4):
            submit(); t.wait()
        if name == "fed":
            assert not t.down_feed_report["status"].any()
        objs[leg] = (t, submit)
    out = {k: {"interval_ms": [], "last_ms": []} for k in objs}
    for _ in range(args.rounds):
        for name, (t, submit) in objs.items():
            iv, dev = np.empty(args.ticks), np.empty(args.ticks)
            submit()
            t0 = time.perf_counter()
            for i in range(args.ticks):
                if i + 1 < args.ticks:
                    submit()
                t.wait()
                t1 = time.perf_counter()
                iv[i], dev[i], t0 = (t1 - t0) * 1e3, t.last_ms(), t1
            out[name]["interval_ms"].append(float(np.median(iv[1:])))
            out[name]["last_ms"].append(float(np.median(dev)))
    for t, _ in objs.values():
        t.close()
    lines.append("tools/tick_feed_down_cost.py on %s: %d streams of 24 kHz stereo 64 kbps psy %d, EDI AF, %d ticks per round and leg with two in flight," % (
        torch.cuda.get_device_name(0), ns, args.psy, args.ticks))
    lines.append("%d rounds interleaved in one process.  Per leg: the rounds' medians of the finished-tick interval (host clock) and of tlb_tick_last_ms (device clock)." % args.rounds)
    lines.append("A 24 kHz frame lasts 48 ms.  Over the link per stream and tick: fed 1160 bytes (two 576-byte slots, two lengths), down 9216, plain 4608.")
    for name in LEGS:
        if name not in out:
            if name in why:
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
    lines.append("(b) fed - down    : interval %+.4f ms, last_ms %+.4f ms; fed - plain: interval %+.4f ms, last_ms %+.4f ms" % (
        med("fed", "interval_ms") - med("down", "interval_ms"), med("fed", "last_ms") - med("down", "last_ms"),
        med("fed", "interval_ms") - med("plain", "interval_ms"), med("fed", "last_ms") - med("plain", "last_ms")))
    for name, p in PARENT_OF.items():
        if args.parent_legs and p in out:
            lines.append("(c) %-5s - %-6s: interval %+.4f ms (the parent leg's spread %.4f ms), last_ms %+.4f ms (spread %.4f ms)" % (
                name, p, med(name, "interval_ms") - med(p, "interval_ms"), max(out[p]["interval_ms"]) - min(out[p]["interval_ms"]),
                med(name, "last_ms") - med(p, "last_ms"), max(out[p]["last_ms"]) - min(out[p]["last_ms"])))
    text = "\n".join(lines) + "\n"
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)
    print(text)


if __name__ == "__main__":
    main()
