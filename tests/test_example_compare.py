"""examples/editick.cpp and examples/nodetick.cpp with --compare: the compare monitor from plain C++.  Both build with a host compiler
alone; on the GPU a short programme-like input gives exit status 0, the monitor's summary line (--compare implies --monitor audio) and the
compare's -- every frame that left was compared and judged, none mismatched, no stream reached a run of 3 -- and the packets are the bytes
of a run without it."""
import re
import subprocess

import pytest

from pcmgen import gen_pcm
from test_example_mp2enc import build

MONITOR = re.compile(r"monitor: (\d+) frames checked, (\d+) bad, longest bad run (\d+), (\d+) (?:stream|service)\(s\) silent at the output")
COMPARE = re.compile(r"compare: (\d+) frames compared, (\d+) judged, (\d+) mismatched, (\d+) alarm\(s\)")


def test_examples_with_the_compare_option_build_with_a_host_compiler(tmp_path):
    for name in ("editick", "nodetick"):
        assert build(tmp_path, name).exists()
        src = (build.__globals__["ROOT"] / "examples" / (name + ".cpp")).read_text()
        assert "--compare" in src and "mismatch_run == 3" in src


@pytest.mark.gpu
def test_editick_compare_summary(tmp_path):
    exe = build(tmp_path, "editick")
    nframes, nstreams = 12, 5
    pcm = gen_pcm(93, 0, 0, nframes)
    (tmp_path / "in.pcm").write_bytes(pcm.transpose(0, 2, 1).reshape(nframes, -1).astype("<i2").tobytes())
    args = [str(exe), str(tmp_path / "in.pcm"), str(tmp_path / "out.af"), "-b", "128", "-m", "j", "-n", str(nstreams)]
    r = subprocess.run(args + ["--compare"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    m, c = MONITOR.search(r.stderr), COMPARE.search(r.stderr)
    assert m and c, r.stderr
    assert [int(x) for x in m.groups()] == [nframes * nstreams, 0, 0, 0]
    assert [int(x) for x in c.groups()] == [nframes * nstreams, nframes * nstreams, 0, 0] and "in a row" not in r.stderr
    first = subprocess.run(args[:3] + ["--compare"] + args[3:], capture_output=True, text=True)      # the flag ahead of the valued options
    assert first.returncode == 0 and COMPARE.search(first.stderr)
    plain = tmp_path / "plain.af"
    r2 = subprocess.run(args[:2] + [str(plain)] + args[3:], capture_output=True, text=True)
    assert r2.returncode == 0 and not COMPARE.search(r2.stderr) and not MONITOR.search(r2.stderr)
    assert plain.read_bytes() == (tmp_path / "out.af").read_bytes()
    assert subprocess.run(args + ["--monitor", "check", "--compare"], capture_output=True, text=True).returncode != 0
    assert subprocess.run(args + ["-b"], capture_output=True, text=True).returncode != 0


@pytest.mark.gpu
def test_nodetick_compare_summary(tmp_path):
    exe = build(tmp_path, "nodetick")
    nin, ns, ticks = 30, 11, 12
    pcm = gen_pcm(124, 0, 0, nin)
    (tmp_path / "in.pcm").write_bytes(pcm.transpose(0, 2, 1).reshape(nin, 2304).astype("<i2").tobytes())
    r = subprocess.run([str(exe), str(tmp_path / "in.pcm"), "-n", str(ns), "-d", "0,0", "-k", str(ticks), "--compare"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    m, c = MONITOR.search(r.stderr), COMPARE.search(r.stderr)
    assert m and c, r.stderr
    assert [int(x) for x in m.groups()] == [ns * ticks, 0, 0, 0]
    assert [int(x) for x in c.groups()] == [ns * ticks, ns * ticks, 0, 0] and "in a row" not in r.stderr
