"""examples/editick.cpp and examples/nodetick.cpp with --source-rate: the device resampler from plain C++.  Both build with a host compiler
alone; on the GPU a 44.1 kHz file fed with --source-rate 44100 gives the packets of the oracle-resampled 48 kHz file fed without the flag,
byte for byte."""
import subprocess

import numpy as np
import pytest

import resamplelib as R
from test_example_mp2enc import build


def test_examples_with_the_source_rate_option_build_with_a_host_compiler(tmp_path):
    for name, call in (("editick", "tlb_tick_need"), ("nodetick", "tlb_node_need")):
        assert build(tmp_path, name).exists()
        src = (build.__globals__["ROOT"] / "examples" / (name + ".cpp")).read_text()
        assert "--source-rate" in src and call in src


@pytest.mark.gpu
def test_editick_source_rate_equals_the_oracle_s_resampled_input(tmp_path):
    exe = build(tmp_path, "editick")
    cfg = dict(samplerate=48000, mode="j", source=44100)
    nframes = 6
    sig = R.signal(cfg, "noise", R.total_need(cfg, nframes), seed=5) // 4
    want = R.Oracle([cfg]).resample(R.cut([sig], [cfg], 0, nframes))
    (tmp_path / "in441.pcm").write_bytes(sig.astype("<i2").tobytes())
    (tmp_path / "in48.pcm").write_bytes(want[:, 0].astype("<i2").tobytes())
    tail = ["-b", "128", "-m", "j", "-n", "3"]
    a = subprocess.run([str(exe), str(tmp_path / "in441.pcm"), str(tmp_path / "a.af")] + tail + ["--source-rate", "44100"], capture_output=True, text=True)
    b = subprocess.run([str(exe), str(tmp_path / "in48.pcm"), str(tmp_path / "b.af")] + tail, capture_output=True, text=True)
    assert a.returncode == 0 and b.returncode == 0, (a.stderr, b.stderr)
    assert "%d ticks" % nframes in a.stderr and "%d ticks" % nframes in b.stderr
    got = (tmp_path / "a.af").read_bytes()
    assert len(got) > nframes * 384 and got == (tmp_path / "b.af").read_bytes()
    bad = subprocess.run([str(exe), str(tmp_path / "in441.pcm"), str(tmp_path / "c.af")] + tail + ["--source-rate", "48001"], capture_output=True, text=True)
    assert bad.returncode != 0


@pytest.mark.gpu
def test_nodetick_source_rate_equals_the_oracle_s_resampled_input(tmp_path):
    """two services on two shards of one GPU; -o writes the LAST service, which starts at source frame 1152 -- without the flag it starts at
    frame 1 of its file, so the 48 kHz file is one frame of anything followed by the oracle's output for the source from frame 1152 on"""
    exe = build(tmp_path, "nodetick")
    cfg = dict(samplerate=48000, mode="j", source=44100)
    ticks = 6
    sig = R.signal(cfg, "noise", 2304 * 4, seed=6) // 4              # whole 2304-value pieces, as the example reads its file; longer than the run needs
    want = R.Oracle([cfg]).resample(R.cut([sig[1152:]], [cfg], 0, ticks))
    (tmp_path / "in441.pcm").write_bytes(sig.astype("<i2").tobytes())
    (tmp_path / "in48.pcm").write_bytes(np.concatenate([np.zeros(2304, np.int16), want[:, 0].reshape(-1)]).astype("<i2").tobytes())
    tail = ["-n", "2", "-d", "0,0", "-k", str(ticks)]
    a = subprocess.run([str(exe), str(tmp_path / "in441.pcm")] + tail + ["-o", str(tmp_path / "a.af"), "--source-rate", "44100"], capture_output=True, text=True)
    b = subprocess.run([str(exe), str(tmp_path / "in48.pcm")] + tail + ["-o", str(tmp_path / "b.af")], capture_output=True, text=True)
    assert a.returncode == 0 and b.returncode == 0, (a.stderr, b.stderr)
    got = (tmp_path / "a.af").read_bytes()
    assert len(got) > (ticks - 2) * 384 and got == (tmp_path / "b.af").read_bytes()
