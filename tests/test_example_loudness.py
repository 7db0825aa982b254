"""examples/editick.cpp and examples/nodetick.cpp with --loudness: the loudness meter from plain C++.  Both must build with a host compiler
alone; on the GPU editick prints, per stream, what the binding computes for the same PCM and gain (Batch.ingest, then Batch.loudness and
Batch.loudness_programme), and its packets do not notice the meter."""
import re
import subprocess

import numpy as np
import pytest

from pcmgen import gen_pcm
from test_example_mp2enc import build

LINE = re.compile(r"loudness: (?:stream|service) (\d+): momentary (\S+) LUFS, short-term (\S+) LUFS, integrated (\S+) LUFS \((\d+) of (\d+) blocks\)")


def test_examples_with_the_loudness_option_build_with_a_host_compiler(tmp_path):
    for name in ("editick", "nodetick"):
        assert build(tmp_path, name).exists()
        assert "--loudness" in (build.__globals__["ROOT"] / "examples" / (name + ".cpp")).read_text()


@pytest.mark.gpu
@pytest.mark.parametrize("fs,channels,mode,kbps,nstreams,gain", [(48000, 2, "j", 128, 3, -6.0), (24000, 1, "m", 64, 2, 0.0)])
def test_editick_prints_what_the_binding_computes(tmp_path, fs, channels, mode, kbps, nstreams, gain):
    import odr_audioenc_amd as M
    exe = build(tmp_path, "editick")
    nframes = 24                                                     # 27 648 samples: 5 bins at 48 kHz, 11 at 24 kHz -- momentary and integrated exist, short-term does not
    pcm = gen_pcm(193, 0, 0, nframes)
    inter = np.zeros((nframes, 2304), dtype=np.int16)
    inter[:, :1152 * channels] = pcm[:, :channels].transpose(0, 2, 1).reshape(nframes, -1)
    (tmp_path / "in.pcm").write_bytes(inter[:, :1152 * channels].astype("<i2").tobytes())
    args = [str(exe), str(tmp_path / "in.pcm"), str(tmp_path / "out.af"), "-r", str(fs), "-c", str(channels), "-b", str(kbps), "-m", mode, "-n", str(nstreams), "-g", str(gain)]
    r = subprocess.run(args + ["--loudness"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = LINE.findall(r.stderr)
    assert [int(g[0]) for g in got] == list(range(nstreams)), r.stderr
    b = M.Batch([M.StreamConfig(samplerate=fs, mode=mode, bitrate=kbps, psy_model=1)] * nstreams)
    b.set_gain_db(gain)
    b.enable_loudness()
    planar, _ = b.ingest(np.repeat(inter[:, None], nstreams, axis=1))
    rec, prog = b.loudness(planar), b.loudness_programme()
    b.close()
    assert (rec["momentary"] > 0).all() and (prog["integrated"] > 0).all() and not rec["short_term"].any()
    for s in range(nstreams):
        want = ("%.2f" % M.loudness_lufs(rec["momentary"][s]), "%.2f" % M.loudness_lufs(rec["short_term"][s]), "%.2f" % M.loudness_lufs(prog["integrated"][s]),
                str(int(prog["gated"][s])), str(int(rec["blocks"][s])))
        assert got[s][1:] == want, (s, got[s], want)
    assert got[0][2] == "-inf"
    plain = tmp_path / "plain.af"
    r2 = subprocess.run(args[:2] + [str(plain)] + args[3:], capture_output=True, text=True)
    assert r2.returncode == 0 and not LINE.search(r2.stderr)
    assert plain.read_bytes() == (tmp_path / "out.af").read_bytes()          # the packets do not notice the meter
