#!/usr/bin/env python3
"""Decode throughput beside the encode rate of the SAME process on the same device: BASELINE configs[1] (4096 streams x 32 frames, 48 kHz
stereo 128 kbps, psy 1), buffers resident on the device: tlb_encode_device_len, then tlb_decode_device with the report only and with
report + PCM.  Prints one line per leg (median of `--reps` timed calls after one warm-up).  tools/decode_first.sh runs it plain and under
rocprofv3 --kernel-trace --stats."""
import argparse
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    torch.cuda.init()
    import odr_audioenc_amd as M
    from pcmgen import gen_pcm
    ns, nf, nbase = a.streams, a.frames, 64
    base = np.stack([gen_pcm(s, 0, 0, nf) for s in range(nbase)], axis=1)
    pcm = np.tile(base, (1, ns // nbase, 1, 1))
    b = M.Batch([M.StreamConfig(mode="s", psy_model=1)] * ns)
    dev = torch.device("cuda:0")
    d_pcm = torch.from_numpy(pcm).to(dev)
    d_out = torch.zeros((nf, ns, b.out_stride), dtype=torch.uint8, device=dev)
    d_len = torch.zeros((nf, ns), dtype=torch.int32, device=dev)
    d_rep = torch.zeros((nf, ns, M.FRAME_REPORT_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    d_dec = torch.zeros((nf, ns, 2, 1152), dtype=torch.int16, device=dev)

    def enc():
        assert b.L.tlb_encode_device_len(b.h, d_pcm.data_ptr(), nf, None, None, d_out.data_ptr(), d_len.data_ptr(), None) == 0

    def dec(with_pcm):
        b.decode_device(d_out.data_ptr(), d_len.data_ptr(), nf, d_rep.data_ptr(), None, d_dec.data_ptr() if with_pcm else None)

    def rate(fn):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t)
        return ns * nf / float(np.median(ts)), ts

    print(f"device: {torch.cuda.get_device_name(0)}; {ns} streams x {nf} frames per call, median of {a.reps} calls")
    for name, fn in (("encode, psy 1 (tlb_encode_device_len)", enc), ("decode, report only", lambda: dec(False)), ("decode, report + PCM", lambda: dec(True))):
        r, ts = rate(fn)
        print(f"{name:40s} {r / 1e6:8.2f} M frames/s   ({min(ts) * 1e3:.2f} .. {max(ts) * 1e3:.2f} ms per call)")
    print(f"frames with a BAD flag: {b.decode_bad_frames()}")
    b.close()


if __name__ == "__main__":
    main()
