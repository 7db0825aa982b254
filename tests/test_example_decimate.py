"""examples/editick.cpp and examples/nodetick.cpp with --source-rate above the service's rate: the device decimator from plain C++.  Both
build with a host compiler alone; on the GPU a 48 kHz file fed with --source-rate 48000 to 24 kHz services gives the packets of the
oracle-decimated 24 kHz file fed without the flag, byte for byte."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import decimatelib as D

ROOT = Path(__file__).resolve().parent.parent
CFG = dict(samplerate=24000, mode="j", source=48000)


def build(tmp_path, name):
    import odr_audioenc_amd as M
    if not M.LIB_PATH.exists():
        M.build()
    exe = tmp_path / name
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", str(ROOT / "examples" / (name + ".cpp")), "-I" + str(ROOT / "include"),
                    "-L" + str(ROOT / "odr-audioenc_amd"), "-ltoolame_dab_hip", "-Wl,-rpath," + str(ROOT / "odr-audioenc_amd"), "-o", str(exe)], check=True)
    return exe


def test_examples_with_a_down_source_build_with_a_host_compiler(tmp_path):
    for name, calls in (("editick", ("tlb_tick_set_down_source", "tlb_tick_down_need", "tlb_tick_down(")), ("nodetick", ("tlb_node_set_down_source", "tlb_node_down_need", "tlb_node_down("))):
        assert build(tmp_path, name).exists()
        src = (ROOT / "examples" / (name + ".cpp")).read_text()
        assert "--source-rate" in src and all(c in src for c in calls)


@pytest.mark.gpu
def test_editick_down_source_equals_the_oracle_s_decimated_input(tmp_path):
    exe = build(tmp_path, "editick")
    nframes = 6
    sig = D.signal(CFG, "noise", D.total_need(CFG, nframes), seed=5) // 4
    want = D.Oracle([CFG]).decimate(D.cut([sig], [CFG], 0, nframes))
    (tmp_path / "in48.pcm").write_bytes(sig.astype("<i2").tobytes())
    (tmp_path / "in24.pcm").write_bytes(want[:, 0].astype("<i2").tobytes())
    tail = ["-r", "24000", "-b", "64", "-m", "j", "-n", "3"]
    a = subprocess.run([str(exe), str(tmp_path / "in48.pcm"), str(tmp_path / "a.af")] + tail + ["--source-rate", "48000"], capture_output=True, text=True)
    b = subprocess.run([str(exe), str(tmp_path / "in24.pcm"), str(tmp_path / "b.af")] + tail, capture_output=True, text=True)
    assert a.returncode == 0 and b.returncode == 0, (a.stderr, b.stderr)
    assert "%d ticks" % nframes in a.stderr and "%d ticks" % nframes in b.stderr
    got = (tmp_path / "a.af").read_bytes()
    assert len(got) > nframes * 384 and got == (tmp_path / "b.af").read_bytes()
    bad = subprocess.run([str(exe), str(tmp_path / "in48.pcm"), str(tmp_path / "c.af")] + tail + ["--source-rate", "48001"], capture_output=True, text=True)
    assert bad.returncode != 0


@pytest.mark.gpu
def test_nodetick_down_source_equals_the_oracle_s_decimated_input(tmp_path):
    """two 24 kHz services on two shards of one GPU; -o writes the LAST service, which starts at source frame 1152 -- without the flag it
    starts at frame 1 of its file, so the 24 kHz file is one frame of anything followed by the oracle's output for the source from frame
    1152 on"""
    exe = build(tmp_path, "nodetick")
    ticks = 6
    sig = D.signal(CFG, "noise", 2304 * (ticks + 1), seed=6) // 4    # whole 2304-value pieces, as the example reads its file; 1152 + 6 x 2304 frames are needed
    want = D.Oracle([CFG]).decimate(D.cut([sig[1152:]], [CFG], 0, ticks))
    (tmp_path / "in48.pcm").write_bytes(sig.astype("<i2").tobytes())
    (tmp_path / "in24.pcm").write_bytes(np.concatenate([np.zeros(2304, np.int16), want[:, 0].reshape(-1)]).astype("<i2").tobytes())
    tail = ["-n", "2", "-d", "0,0", "-k", str(ticks), "-r", "24000", "-b", "64"]
    a = subprocess.run([str(exe), str(tmp_path / "in48.pcm")] + tail + ["-o", str(tmp_path / "a.af"), "--source-rate", "48000"], capture_output=True, text=True)
    b = subprocess.run([str(exe), str(tmp_path / "in24.pcm")] + tail + ["-o", str(tmp_path / "b.af")], capture_output=True, text=True)
    assert a.returncode == 0 and b.returncode == 0, (a.stderr, b.stderr)
    got = (tmp_path / "a.af").read_bytes()
    assert len(got) > (ticks - 2) * 384 and got == (tmp_path / "b.af").read_bytes()
