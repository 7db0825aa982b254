"""examples/editick.cpp and examples/nodetick.cpp with --limit: the true-peak limiter from plain C++.  Both must build with a host compiler
alone; on the GPU editick --limit -1 on a hot input -- a full-scale sine at fs / 4 sampled 45 degrees off its crests, 3 dB over full
scale in true peak -- prints, per stream, the counters the binding computes for the same PCM (Batch.ingest, then Batch.limit), and its
packets are those of the limited PCM, not of the input."""
import math
import re
import subprocess

import numpy as np
import pytest

import truepeaklib as TP
from test_example_mp2enc import build

LINE = re.compile(r"limiter: (?:stream|service) (\d+): limited (\d+) of (\d+) frames, red_max (\d+) \((\S+) dB\), input max (\S+) dBTP, ceiling (\S+) dBTP")
N = 1152


def test_examples_with_the_limit_option_build_with_a_host_compiler(tmp_path):
    for name in ("editick", "nodetick"):
        assert build(tmp_path, name).exists()
        text = (build.__globals__["ROOT"] / "examples" / (name + ".cpp")).read_text()
        assert "--limit" in text and "--limit-release" in text


def _hot(nframes):
    """int16 [nframes][2304] interleaved stereo: fs / 4 at 45 degrees at full scale, quiet in the last two frames"""
    x = TP.sine(0.25, math.pi / 4.0, math.sqrt(2.0), nframes * N).reshape(nframes, N)
    x[-2:] //= 16
    inter = np.zeros((nframes, 2 * N), dtype=np.int16)
    inter[:, 0::2] = x
    inter[:, 1::2] = x // 2
    return inter


@pytest.mark.gpu
@pytest.mark.parametrize("opt,ceiling_db,release", [(["--limit", "-1"], -1.0, 0), (["--limit", "-6", "--limit-release", "10"], -6.0, 10)], ids=["-1 dBTP", "-6 dBTP 10 ms"])
def test_editick_prints_what_the_binding_computes(tmp_path, opt, ceiling_db, release):
    import odr_audioenc_amd as M
    exe = build(tmp_path, "editick")
    nframes, nstreams = 6, 2
    inter = _hot(nframes)
    (tmp_path / "in.pcm").write_bytes(inter.astype("<i2").tobytes())
    args = [str(exe), str(tmp_path / "in.pcm"), str(tmp_path / "out.af"), "-r", "48000", "-c", "2", "-b", "128", "-m", "s", "-n", str(nstreams)]
    r = subprocess.run(args + opt, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = LINE.findall(r.stderr)
    assert [int(g[0]) for g in got] == list(range(nstreams)), r.stderr
    ceiling = int(round(2.0 ** 30 * 10.0 ** (ceiling_db / 20.0)))
    b = M.Batch([M.StreamConfig(samplerate=48000, mode="s", bitrate=128, psy_model=1)] * nstreams)
    b.enable_limiter(ceiling, release)
    planar, _ = b.ingest(np.repeat(inter[:, None], nstreams, axis=1))
    _, rec = b.limit(planar)
    b.close()
    for s in range(nstreams):
        want = (str(int(rec["limited"][s])), str(int(rec["frames"][s])), str(int(rec["red_max"][s])),
                "%.2f" % (20.0 * math.log10((65536.0 - int(rec["red_max"][s])) / 65536.0)), "%.2f" % M.truepeak_dbtp(int(rec["peak_in_max"][s])), "%.2f" % M.truepeak_dbtp(ceiling))
        assert got[s][1:] == want, (s, got[s], want)
    assert int(got[0][2]) == nframes and 4 <= int(got[0][1]) <= nframes and abs(float(got[0][5]) - 3.0) <= 0.15
    assert abs(float(got[0][4]) - (ceiling_db - 3.0)) <= 0.2         # 3 dB over full scale in true peak comes down to the ceiling
    plain = tmp_path / "plain.af"
    r2 = subprocess.run(args[:2] + [str(plain)] + args[3:], capture_output=True, text=True)
    assert r2.returncode == 0 and not LINE.search(r2.stderr)
    assert plain.read_bytes() != (tmp_path / "out.af").read_bytes()          # what is encoded is the limited PCM
