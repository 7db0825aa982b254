"""examples/editick.cpp and examples/nodetick.cpp with --truepeak: the true-peak meter from plain C++.  Both must build with a host compiler
alone; on the GPU they print, per stream, what the binding computes for the same PCM (Batch.ingest, then Batch.truepeak) -- a sine at
fs / 4 sampled 45 degrees off its crests, whose samples show 3 dB less than its true peak -- and editick's packets do not notice the
meter."""
import math
import re
import subprocess

import numpy as np
import pytest

import truepeaklib as TP
from test_example_mp2enc import build

LINE = re.compile(r"truepeak: (?:stream|service) (\d+): max (\S+) dBTP, samples (\S+) dBFS, (\d+) of (\d+) frames over (\S+) dBTP")
N = 1152


def test_examples_with_the_truepeak_option_build_with_a_host_compiler(tmp_path):
    for name in ("editick", "nodetick"):
        assert build(tmp_path, name).exists()
        assert "--truepeak" in (build.__globals__["ROOT"] / "examples" / (name + ".cpp")).read_text()


def _sine(nframes, amp):
    """int16 [nframes][2304] interleaved stereo: fs / 4 at 45 degrees, the right channel 6 dB under the left"""
    x = TP.sine(0.25, math.pi / 4.0, amp, nframes * N).reshape(nframes, N)
    inter = np.zeros((nframes, 2 * N), dtype=np.int16)
    inter[:, 0::2] = x
    inter[:, 1::2] = x // 2
    return inter


def _want(M, rec, s, ceiling_db):
    pk, sm = int(rec["peak_max"][s].max()), int(rec["sample_max"][s].max())
    ceiling = int(round(2.0 ** 30 * 10.0 ** (ceiling_db / 20.0)))
    return ("%.2f" % M.truepeak_dbtp(pk), "%.2f" % M.truepeak_dbtp(sm << 15), str(int(rec["overs"][s])), str(int(rec["frames"][s])), "%.2f" % M.truepeak_dbtp(ceiling))


@pytest.mark.gpu
@pytest.mark.parametrize("opt,ceiling_db", [(["--truepeak"], -1.0), (["--truepeak", "-4.5"], -4.5)])
def test_editick_prints_what_the_binding_computes(tmp_path, opt, ceiling_db):
    import odr_audioenc_amd as M
    exe = build(tmp_path, "editick")
    nframes, nstreams = 6, 2
    inter = _sine(nframes, 10.0 ** (-3.0 / 20.0))                    # true peak -3 dBTP, sample peaks -6 dBFS: over -4.5 dBTP, under -1
    (tmp_path / "in.pcm").write_bytes(inter.astype("<i2").tobytes())
    args = [str(exe), str(tmp_path / "in.pcm"), str(tmp_path / "out.af"), "-r", "48000", "-c", "2", "-b", "128", "-m", "s", "-n", str(nstreams)]
    r = subprocess.run(args + opt, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = LINE.findall(r.stderr)
    assert [int(g[0]) for g in got] == list(range(nstreams)), r.stderr
    b = M.Batch([M.StreamConfig(samplerate=48000, mode="s", bitrate=128, psy_model=1)] * nstreams)
    b.enable_truepeak(int(round(2.0 ** 30 * 10.0 ** (ceiling_db / 20.0))))
    planar, _ = b.ingest(np.repeat(inter[:, None], nstreams, axis=1))
    rec = b.truepeak(planar)
    b.close()
    for s in range(nstreams):
        assert got[s][1:] == _want(M, rec, s, ceiling_db), (s, got[s])
    assert abs(float(got[0][1]) - (-3.0)) <= 0.15 and abs(float(got[0][2]) - (-6.01)) <= 0.05      # (the abrupt onset overshoots by 0.1 dB: a real peak)
    assert int(got[0][3]) == (nframes if ceiling_db < -3.0 else 0) and int(got[0][4]) == nframes
    plain = tmp_path / "plain.af"
    r2 = subprocess.run(args[:2] + [str(plain)] + args[3:], capture_output=True, text=True)
    assert r2.returncode == 0 and not LINE.search(r2.stderr)
    assert plain.read_bytes() == (tmp_path / "out.af").read_bytes()          # the packets do not notice the meter


@pytest.mark.gpu
def test_nodetick_prints_what_the_binding_computes(tmp_path):
    import odr_audioenc_amd as M
    exe = build(tmp_path, "nodetick")
    nframes, nstreams, ticks = 5, 3, 4
    inter = _sine(nframes, 10.0 ** (-3.0 / 20.0))
    (tmp_path / "in.pcm").write_bytes(inter.astype("<i2").tobytes())
    r = subprocess.run([str(exe), str(tmp_path / "in.pcm"), "-n", str(nstreams), "-G", "2", "-d", "0,0", "-k", str(ticks), "--truepeak"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = LINE.findall(r.stderr)
    assert [int(g[0]) for g in got] == list(range(nstreams)), r.stderr
    b = M.Batch([M.StreamConfig(samplerate=48000, mode="s", bitrate=128, psy_model=1)] * nstreams)
    b.enable_truepeak()
    fed = np.stack([np.stack([inter[(s + t) % nframes] for s in range(nstreams)]) for t in range(ticks)])      # service s takes frame s + t at tick t
    planar, _ = b.ingest(fed)
    rec = b.truepeak(planar)
    b.close()
    for s in range(nstreams):
        assert got[s][1:] == _want(M, rec, s, -1.0), (s, got[s])
    assert abs(float(got[1][1]) - (-3.0)) <= 0.15 and got[1][4] == str(ticks)
