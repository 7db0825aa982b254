"""Host logic: psy model 1 on stereo frames (mp2_psy13.h: tl_psy1_stereo), whose band centres and decimation of both channels run
in one pass on the two halves of the wave (tl_psy1_centres2, tl_psy1_decimate2), executed by the lane-loop emulation (tests/emu)
against the oracle byte for byte.  CPU only.

The paired pass runs when neither channel has a dead head and neither tone list has more than 32 entries.  Longer lists take the
per-channel order after the chains, dead heads the orders tests/test_psy1_pairing.py describes.  A counting build of the emulation
(-DTL_DEBUG_DUMP: emu_back_stats) shows that each of these was taken, and inside the paired pass a band centre that fell on a
tone's line (and moved off it) and two bands of one channel sharing a centre.

One counter stays at zero on every signal, and has to: "a centre still on a tone's line after the move" (index 6), the condition
under which a band's level replaces a tone's.  On frames without a dead head a line is TONE only if it is a confirmed, un-erased
tone; tones are local maxima (strict on one side), so no two TONE lines are adjacent, and the move goes from a TONE line to one of
its two neighbours.  The replacement loop is kept for parity with the per-channel code; the test prints the counter."""
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
from test_psy1_pairing import DEAD_HEAD_CH0, DEAD_HEAD_CH1, NF, STRESS_SEEDS, crafted

ROOT = Path(__file__).resolve().parent.parent


def comb(seed):
    """44 sinusoids per channel, spaced just beyond each other's erasure reach in every run range (2, 3, 6, 12 lines), over a
    quiet noise floor: more than 32 confirmed tones in both channels' lists."""
    rng = np.random.default_rng(seed)
    n = np.arange(NF * 1152)
    lines = list(range(4, 62, 4)) + list(range(66, 127, 6)) + list(range(134, 255, 14)) + list(range(270, 495, 26))
    x = np.zeros((2, NF * 1152))
    for ch in range(2):
        for b in lines:
            x[ch] += 10 ** rng.uniform(2.0, 2.6) * np.sin(2 * np.pi * b * 46.875 * n / 48000 + rng.uniform(0, 6.28))
        x[ch] += rng.normal(0, 0.5, n.shape)
    x = np.clip(np.round(x), -32768, 32767).astype(np.int16)
    return np.ascontiguousarray(x.reshape(2, NF, 1152).transpose(1, 0, 2))


def mixed():
    """the comb in channel 0 only, a stress signal in channel 1: one long list is enough for the per-channel order"""
    p = comb(0)
    p[:, 1] = crafted(3)[:, 1]
    return p


CONFIGS = [(mode, fs, kbps) for mode in ("s", "j", "d") for fs, rates in ((32000, (128, 192)), (44100, (128, 256)), (48000, (128, 384)))
           for kbps in rates]


def _signals():
    sig = [("kind%d" % k, gen_pcm(700 + 13 * k, k, 0, NF)) for k in range(8)]
    sig += [("stress%d" % s, crafted(s)) for s in STRESS_SEEDS + (1, 7)]
    sig += [("comb%d" % s, comb(s)) for s in (0, 1)] + [("mixed", mixed())]
    return sig


@pytest.mark.parametrize("mode,fs,kbps", CONFIGS)
def test_stereo_psy1_back_emulation_matches_oracle(mode, fs, kbps):
    """Every pcmgen kind, the tone-labelling stress signals and the long-list signals, one stream each in one batch, against the
    oracle byte for byte."""
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
L.emu_back_stats.argtypes = [ctypes.c_void_p]
def stats():
    a = (ctypes.c_long * 7)(); L.emu_back_stats(a); return list(a)
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
PAIRED, LONG_LIST, CENTRE_MOVED, SHARED_CENTRE, DEAD0, DEAD1, CENTRE_STAYS_ON_TONE = range(7)


def test_stereo_psy1_back_paths_reached(tmp_path):
    """The counting build runs every signal of the byte comparison in its own process (48 kHz, 's', 128 kbps); every case equals the
    oracle, every frame is booked to exactly one order, and each order and each rare branch of the paired pass was taken."""
    lib = tmp_path / "libmp2emu_dbg.so"
    emu = ROOT / "tests" / "emu"
    csrc = ROOT / "odr-audioenc_amd" / "csrc"
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-mfma", "-ffp-contract=off", "-fno-strict-aliasing", "-w", "-DTL_DEBUG_DUMP",
                    "-shared", "-o", str(lib), str(emu / "mp2_emu.cpp"), str(csrc / "mp2_host.cpp"), "-lm"], check=True)
    cases = {}
    for name, p in _signals():
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
        st = res[name]["stats"]
        print(name, "paired, long list, centres moved, shared centre, dead head 0, dead head 1, centre stays on tone:", st)
        assert st[PAIRED] + st[LONG_LIST] + st[DEAD0] + st[DEAD1] == NF, name
    st = {k: v["stats"] for k, v in res.items()}
    # the paired pass, with a centre that fell on a tone's line and with two bands sharing a centre
    assert all(st["kind%d" % k][PAIRED] == NF for k in range(8))
    assert sum(v[CENTRE_MOVED] for v in st.values()) > 0 and st["kind0"][CENTRE_MOVED] > 0
    assert sum(v[SHARED_CENTRE] for v in st.values()) > 0 and st["stress1"][SHARED_CENTRE] > 0
    # more than 32 entries in a tone list: both channels' lists, and channel 0's alone
    assert st["comb0"][LONG_LIST] > 0 and st["comb1"][LONG_LIST] > 0 and st["mixed"][LONG_LIST] > 0
    # both dead-head orders, next to paired frames of the same stream
    assert st["stress%d" % DEAD_HEAD_CH0][DEAD0] > 0 and st["stress%d" % DEAD_HEAD_CH0][PAIRED] > 0
    assert st["stress%d" % DEAD_HEAD_CH1][DEAD1] > 0 and st["stress%d" % DEAD_HEAD_CH1][PAIRED] > 0
    # see the module's docstring: unreachable without a dead head
    print("centre stays on a tone's line:", sum(v[CENTRE_STAYS_ON_TONE] for v in st.values()))
