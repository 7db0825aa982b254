"""Host logic: psy model 1 on stereo frames (mp2_psy13.h: tl_psy1_stereo), whose band weight sums of both channels run on the
two halves of the wave, executed by the lane-loop emulation (tests/emu) against the oracle byte for byte.  CPU only.

The weight sums are paired on the regular path (neither channel's tone list has an erased head).  A dead-head channel 0 takes
the plain per-channel order; a dead-head channel 1 is finished first and channel 0's parked levels AND weight terms return to
the LDS arrays for its own chain.  The cases below reach all three paths; a debug build of the emulation counts the dead
heads so that the test knows the paths were taken."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import emulib as E
import oraclelib as O
from pcmgen import gen_pcm

ROOT = Path(__file__).resolve().parent.parent
NF = 6


def crafted(seed):
    """tools/fuzz_emu.py's tone-labelling stress signal (range boundaries 63/127/255, near-7-dB neighbours, adjacent tones,
    head erasure), restated here so that the test does not depend on a tool script."""
    rng = np.random.default_rng(seed)
    n = np.arange(NF * 1152)
    x = np.zeros((2, NF * 1152))
    ntones = rng.integers(2, 40)
    anchors = np.array([2, 3, 4, 60, 61, 62, 63, 64, 66, 124, 126, 127, 128, 130, 133, 250, 254, 255, 256, 262, 268, 280, 400, 487, 495, 499])
    for ch in range(2):
        for _ in range(ntones):
            if rng.random() < 0.6:
                b = float(rng.choice(anchors)) + rng.choice([0, 0, 0.5, -0.25, 0.25])
            else:
                b = rng.uniform(1, 510)
            if rng.random() < 0.5:
                b2 = b + rng.integers(1, 14)
                amp2 = 10 ** rng.uniform(0.5, 4.2)
                x[ch] += amp2 * np.sin(2 * np.pi * b2 * 46.875 * n / 48000 + rng.uniform(0, 6.28))
            amp = 10 ** rng.uniform(0.5, 4.2)
            x[ch] += amp * np.sin(2 * np.pi * b * 46.875 * n / 48000 + rng.uniform(0, 6.28))
        x[ch] += rng.normal(0, 10 ** rng.uniform(-0.5, 3), n.shape)
    x = np.clip(np.round(x), -32768, 32767).astype(np.int16)
    return np.ascontiguousarray(x.reshape(2, NF, 1152).transpose(1, 0, 2))


# Chosen on the host with a counting build of the emulation (not by the code under test): at 48 kHz, 's', 128 kbps the stress
# signal of seed 94 has a dead head in channel 0 only, that of seed 28 in channel 1 only (each checked with the other channel
# silenced); the other seeds add tone-rich frames with erased tones.
DEAD_HEAD_CH0, DEAD_HEAD_CH1 = 94, 28
STRESS_SEEDS = (DEAD_HEAD_CH0, DEAD_HEAD_CH1, 0, 2, 4, 112, 222, 380)
CONFIGS = [(mode, fs, kbps) for mode in ("s", "j", "d") for fs, rates in ((32000, (128, 192)), (44100, (128, 256)), (48000, (128, 384)))
           for kbps in rates]


def _signals():
    sig = [("kind%d" % k, gen_pcm(700 + 13 * k, k, 0, NF)) for k in range(8)]
    sig += [("stress%d" % s, crafted(s)) for s in STRESS_SEEDS]
    return sig


@pytest.mark.parametrize("mode,fs,kbps", CONFIGS)
def test_stereo_psy1_emulation_matches_oracle(mode, fs, kbps):
    """Every pcmgen kind and the stress signals, one stream each in one batch, against the oracle byte for byte."""
    sig = _signals()
    b = E.EmuBatch([dict(samplerate=fs, mode=mode, kbps=kbps, psy=1)] * len(sig))
    got, _ = b.encode(np.stack([p for _, p in sig], axis=1))
    tail = b.flush()
    b.close()
    for s, (name, pcm) in enumerate(sig):
        ref, _ = O.oracle_stream(pcm, samplerate=fs, mode=mode, kbps=kbps, psy=1)
        assert len(ref) > 0, name
        assert got[s] + tail[s] == ref, (name, mode, fs, kbps)


_COUNT = r"""
import ctypes, json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import emulib as E
L = E.lib()
L.emu_walk_stats.argtypes = [ctypes.c_void_p]
def stats():
    a = (ctypes.c_long * 5)(); L.emu_walk_stats(a); return list(a)
res = {}
for name, path in json.loads(sys.argv[2]).items():
    pcm = np.load(path)
    s0 = stats()
    b = E.EmuBatch([dict(samplerate=48000, mode="s", kbps=128, psy=1)])
    got, _ = b.encode(pcm[:, None]); out = got[0] + b.flush()[0]; b.close()
    s1 = stats()
    res[name] = dict(stats=[y - x for x, y in zip(s0, s1)], out=out.hex())
print(json.dumps(res))
"""


def test_stereo_psy1_paths_reached(tmp_path):
    """A counting build of the emulation (-DTL_DEBUG_DUMP: emu_walk_stats = rounds, tones, dead heads, fronts, candidates) runs the
    dead-head cases in their own process.  Channel 0 alone (channel 1 silent) and channel 1 alone show which channel carries the
    dead head; the full stereo signal then takes that channel's path.  Every case equals the oracle."""
    lib = tmp_path / "libmp2emu_dbg.so"
    emu = ROOT / "tests" / "emu"
    csrc = ROOT / "odr-audioenc_amd" / "csrc"
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-mfma", "-ffp-contract=off", "-fno-strict-aliasing", "-w", "-DTL_DEBUG_DUMP",
                    "-shared", "-o", str(lib), str(emu / "mp2_emu.cpp"), str(csrc / "mp2_host.cpp"), "-lm"], check=True)
    cases = {}
    for tag, seed in (("ch0", DEAD_HEAD_CH0), ("ch1", DEAD_HEAD_CH1)):
        pcm = crafted(seed)
        only0, only1 = pcm.copy(), pcm.copy()
        only0[:, 1] = 0
        only1[:, 0] = 0
        for name, p in ((tag + "_stereo", pcm), (tag + "_only0", only0), (tag + "_only1", only1)):
            path = tmp_path / (name + ".npy")
            np.save(path, p)
            cases[name] = (str(path), p)
    env = dict(os.environ, TL_EMU_LIB=str(lib))
    r = subprocess.run([sys.executable, "-c", _COUNT, str(ROOT / "tests"), json.dumps({k: v[0] for k, v in cases.items()})],
                       env=env, capture_output=True, text=True, check=True)
    res = json.loads(r.stdout.strip().splitlines()[-1])
    for name, (_, p) in cases.items():
        ref, _ = O.oracle_stream(p, samplerate=48000, mode="s", kbps=128, psy=1)
        assert len(ref) > 0, name
        assert bytes.fromhex(res[name]["out"]) == ref, name
        print(name, "rounds, tones, dead heads, fronts, candidates:", res[name]["stats"])
    dead = {k: v["stats"][2] for k, v in res.items()}
    # channel 0's dead head: the plain per-channel order
    assert dead["ch0_only0"] > 0 and dead["ch0_only1"] == 0 and dead["ch0_stereo"] > 0
    # channel 1's dead head with a regular channel 0: channel 0's parked terms return for its own chain
    assert dead["ch1_only1"] > 0 and dead["ch1_only0"] == 0 and dead["ch1_stereo"] > 0
    # the paired path: two fronts per stereo frame, most of them regular; an erased head implies erased tones
    for k, v in res.items():
        assert v["stats"][3] == 2 * NF, k
        assert v["stats"][1] > 0, k
