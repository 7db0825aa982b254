"""examples/editick.cpp and examples/nodetick.cpp with --lra: the loudness range from plain C++.  Both must build with a host compiler
alone; on the GPU each prints, per stream, what the oracle of tests/lralib.py gives for a two-level file, behind loudness lines that are
character for character those of a run with --loudness alone; without either option nothing of it is printed and the packets are the same."""
import math
import re
import subprocess

import numpy as np
import pytest

import loudnesslib as LL
import lralib as RL
from test_example_mp2enc import build

LINE = re.compile(r"lra: (?:stream|service) (\d+): LRA (\S+) LU, low (\S+) LUFS, high (\S+) LUFS \((\d+) of (\d+) blocks\)")
LOUD = re.compile(r"^.*loudness: (?:stream|service) \d+: .*$", re.M)
FS, NF = 24000, 80                                                   # 92 160 samples a channel: 38 bins, 9 range blocks


def test_examples_with_the_lra_option_build_with_a_host_compiler(tmp_path):
    for name in ("editick", "nodetick"):
        assert build(tmp_path, name).exists()
        assert "--lra" in (build.__globals__["ROOT"] / "examples" / (name + ".cpp")).read_text()


@pytest.fixture(scope="module")
def two_level():
    """the file, int16 [80][2304] interleaved stereo: a 997 Hz sine at -12 dBFS for 40 frames, at -24 dBFS for 40 (the right channel
    inverted); and the oracle's range records of service 0 (the file from its start) and service 1 (from frame 1, wrapping round)"""
    import odr_audioenc_amd as M
    n = np.arange(NF * 1152)
    v = np.round(32767.0 * np.where(n < 40 * 1152, 10.0 ** (-12 / 20.0), 10.0 ** (-24 / 20.0)) * np.sin(2.0 * math.pi * 997.0 * n / FS)).astype(np.int16)
    inter = np.stack([v, -v], axis=1).reshape(NF, 2304)
    fed = np.stack([inter, np.roll(inter, -1, axis=0)], axis=1)      # [tick][service][2304]
    cfgs = [dict(samplerate=FS, mode="j", kbps=64)] * 2
    b = M.Batch(LL.stream_configs(cfgs))
    planar, _ = b.ingest(fed)
    b.close()
    o = RL.Oracle(cfgs)
    o.loudness(planar)
    want = o.lra()
    assert (want["blocks"] == 9).all() and (want["high_bin"] > want["low_bin"]).all()
    return inter, want


def _want(rec):
    return ("%.1f" % RL.lu(rec), "%.2f" % LL.lufs(float(rec["low"])), "%.2f" % LL.lufs(float(rec["high"])), str(int(rec["gated"])), str(int(rec["blocks"])))


@pytest.mark.gpu
def test_editick_prints_the_oracle_s_range(tmp_path, two_level):
    inter, want = two_level
    exe = build(tmp_path, "editick")
    (tmp_path / "in.pcm").write_bytes(inter.astype("<i2").tobytes())
    runs = {}
    for opt in ("--lra", "--loudness", None):
        out = tmp_path / ("out%s.af" % (opt or ""))
        r = subprocess.run([str(exe), str(tmp_path / "in.pcm"), str(out), "-r", str(FS), "-c", "2", "-b", "64", "-m", "j", "-n", "2"] + ([opt] if opt else []),
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        runs[opt] = (r.stderr, out.read_bytes())
    got = LINE.findall(runs["--lra"][0])
    assert [int(g[0]) for g in got] == [0, 1], runs["--lra"][0]
    for s in range(2):
        assert got[s][1:] == _want(want[0]), (s, got[s], _want(want[0]))             # both streams read the file from its start
    assert LOUD.findall(runs["--lra"][0]) == LOUD.findall(runs["--loudness"][0]) and len(LOUD.findall(runs["--loudness"][0])) == 2
    assert not LINE.search(runs["--loudness"][0]) and not LINE.search(runs[None][0]) and not LOUD.search(runs[None][0])
    assert runs["--lra"][1] == runs["--loudness"][1] == runs[None][1] and len(runs[None][1]) > 0      # the packets do not notice the meter


@pytest.mark.gpu
def test_nodetick_prints_the_oracle_s_range(tmp_path, two_level):
    inter, want = two_level
    exe = build(tmp_path, "nodetick")
    (tmp_path / "in.pcm").write_bytes(inter.astype("<i2").tobytes())
    runs = {}
    for opt in ("--lra", "--loudness"):
        r = subprocess.run([str(exe), str(tmp_path / "in.pcm"), "-n", "2", "-d", "0,0", "-k", str(NF), "-r", str(FS), "-b", "64", "-o", str(tmp_path / "node.af"), opt],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        runs[opt] = (r.stderr, (tmp_path / "node.af").read_bytes())
    got = LINE.findall(runs["--lra"][0])
    assert [int(g[0]) for g in got] == [0, 1], runs["--lra"][0]
    for s in range(2):
        assert got[s][1:] == _want(want[s]), (s, got[s], _want(want[s]))
    assert LOUD.findall(runs["--lra"][0]) == LOUD.findall(runs["--loudness"][0]) and len(LOUD.findall(runs["--loudness"][0])) == 2
    assert not LINE.search(runs["--loudness"][0])
    assert runs["--lra"][1] == runs["--loudness"][1] and len(runs["--lra"][1]) > 0
