"""examples/editick.cpp and examples/nodetick.cpp with --monitor: the confidence monitor from plain C++.  Both must build with a host
compiler alone; on the GPU a short input gives exit status 0 and one summary line -- every frame that left was checked, none was bad."""
import re
import subprocess

import pytest

from pcmgen import gen_pcm
from test_example_mp2enc import build

SUMMARY = re.compile(r"monitor: (\d+) frames checked, (\d+) bad, longest bad run (\d+), (\d+) (?:stream|service)\(s\) silent at the output")


def test_examples_with_the_monitor_option_build_with_a_host_compiler(tmp_path):
    for name in ("editick", "nodetick"):
        assert build(tmp_path, name).exists()
        assert "--monitor" in (build.__globals__["ROOT"] / "examples" / (name + ".cpp")).read_text()


@pytest.mark.gpu
@pytest.mark.parametrize("what,fs,channels,mode,kbps,nstreams", [("audio", 48000, 2, "j", 128, 5), ("check", 24000, 1, "m", 64, 3)])
def test_editick_monitor_summary(tmp_path, what, fs, channels, mode, kbps, nstreams):
    exe = build(tmp_path, "editick")
    nframes = 20
    pcm = gen_pcm(93, 0, 0, nframes)
    (tmp_path / "in.pcm").write_bytes(pcm[:, :channels].transpose(0, 2, 1).reshape(nframes, -1).astype("<i2").tobytes())
    args = [str(exe), str(tmp_path / "in.pcm"), str(tmp_path / "out.af"), "-r", str(fs), "-c", str(channels), "-b", str(kbps), "-m", mode, "-n", str(nstreams)]
    r = subprocess.run(args + ["--monitor", what], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    m = SUMMARY.search(r.stderr)
    assert m, r.stderr
    assert [int(x) for x in m.groups()] == [nframes * nstreams, 0, 0, 0]
    plain = tmp_path / "plain.af"
    r2 = subprocess.run(args[:2] + [str(plain)] + args[3:], capture_output=True, text=True)
    assert r2.returncode == 0 and not SUMMARY.search(r2.stderr)
    assert plain.read_bytes() == (tmp_path / "out.af").read_bytes()          # the packets do not notice the monitor
    bad = subprocess.run(args + ["--monitor", "loud"], capture_output=True, text=True)
    assert bad.returncode != 0


@pytest.mark.gpu
def test_nodetick_monitor_summary(tmp_path):
    exe = build(tmp_path, "nodetick")
    nin, ns, ticks = 30, 11, 12
    pcm = gen_pcm(124, 0, 0, nin)
    (tmp_path / "in.pcm").write_bytes(pcm.transpose(0, 2, 1).reshape(nin, 2304).astype("<i2").tobytes())
    r = subprocess.run([str(exe), str(tmp_path / "in.pcm"), "-n", str(ns), "-d", "0,0", "-k", str(ticks), "--monitor", "audio"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    m = SUMMARY.search(r.stderr)
    assert m, r.stderr
    assert [int(x) for x in m.groups()] == [ns * ticks, 0, 0, 0]
