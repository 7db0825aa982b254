"""The examples with feed concealment on ADAPTED and DOWN feeds: `editick --feed ... --feed-rate 32000 --feed-drop-every 5 --feed-drop-run 2
--conceal` prints the record the drop pattern implies over the WANTED slots (a dropped frame is a wanted slot left empty) and ships what a
tick object with tlb_tick_enable_feed_loss ships; the same for a down feed's record; `nodetick` and `mp2enc --from-mp2 -r R` take the
option too.  Every run of an example is under a time limit of its own."""
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import concealconvlib as V
import conceallib as K

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
NS, EVERY, RUN = 2, 5, 2


def dropped(k):
    return k % EVERY >= EVERY - RUN


def build(tmp_path, name):
    """the example against the library as it stands (built when there is none)"""
    import odr_audioenc_amd as M
    if not M.LIB_PATH.exists():
        M.build()
    exe = tmp_path / name
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", str(ROOT / "examples" / (name + ".cpp")), "-I" + str(ROOT / "include"),
                    "-L" + str(ROOT / "odr-audioenc_amd"), "-ltoolame_dab_hip", "-Wl,-rpath," + str(ROOT / "odr-audioenc_amd"), "-pthread", "-o", str(exe)], check=True)
    return exe


def run(args):
    r = subprocess.run(["timeout", "-k", "10", "60"] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r


@pytest.fixture(scope="module")
def sources(tmp_path_factory):
    """the oracle encoder's sixteen frames at 32 kHz stereo 128 kbps and at 48 kHz stereo 192 kbps as .mp2 files -> {rate: (path, frames)}"""
    d = tmp_path_factory.mktemp("ccvsrc")
    out = {}
    for ci in (0, 4):
        frames = V.case_frames(ci)
        rate = V.CASES[ci][1][0]
        (d / f"{rate}.mp2").write_bytes(b"".join(frames))
        out[rate] = (d / f"{rate}.mp2", frames)
    assert len(out[32000][1]) == len(out[48000][1]) == 16
    return out


def af_packets(path):
    blob, out, o = Path(path).read_bytes(), [], 0
    while o < len(blob):
        k = struct.unpack_from("<I", blob, o)[0]
        out.append(blob[o + 4:o + 4 + k])
        o += 4 + k
    return out


def line(name, ns, nslots):
    rec = K.oracle_record([dropped(k) for k in range(nslots)], 4, 3)
    v = [int(rec[n]) for n in ("frames", "passed", "concealed", "muted", "runs")]
    assert v[0] == nslots and v[2] > 0 and v[3] == 0
    return "%s: conceal: %d slots, %d passed, %d concealed, %d muted, %d runs, longest %d" % ((name,) + tuple(ns * x for x in v) + (int(rec["longest"]),))


def tick_packets(frames, conceal):
    """what one tick object ships for service 0 of editick with the 32 kHz feed: the file's frames on the wanted ticks, the dropped ones' slots empty"""
    import odr_audioenc_amd as M
    t = M.Tick([M.StreamConfig(mode="j", bitrate=128, psy_model=1)], egress="af", version=b"editick example", now_s=1712345678, delay_ms=0, tist=True, tai_utc_offset=37)
    t.set_feed(0, M.FeedConfig(32000, 128, 2), adapt=True)
    if conceal:
        t.enable_conceal(4, 3, any_feed=True)
    out, used = [], 0
    while True:
        want = t.feed_want(0)
        if want and used == len(frames):
            break
        if want and not dropped(used):
            b = frames[used]
            t.feed[0, :len(b)] = np.frombuffer(b, dtype=np.uint8)
            t.feed_len[0] = len(b)
        used += want
        t.run()
        out += t.packets(0)
    t.finish()
    out += t.packets(0)
    t.close()
    return out


def test_editick_conceals_an_adapted_and_a_down_feed(tmp_path, sources):
    exe = build(tmp_path, "editick")
    mp2, frames = sources[32000]
    common = ["-n", NS, "-t", 1712345678, "--feed", mp2, "--feed-bitrate", 128, "--feed-rate", 32000, "--feed-drop-every", EVERY, "--feed-drop-run", RUN]
    r = run([exe, "-", tmp_path / "on.af"] + common + ["--conceal"])
    assert line("editick", NS, 16) in r.stderr, r.stderr
    r = run([exe, "-", tmp_path / "off.af"] + common)
    assert "conceal:" not in r.stderr
    on, off = af_packets(tmp_path / "on.af"), af_packets(tmp_path / "off.af")
    assert on == tick_packets(frames, True) and off == tick_packets(frames, False) and on != off and len(on) == len(off) > 16
    # a down feed: 48 kHz 192 kbps for 24 kHz services, two slots a tick
    mp2, _ = sources[48000]
    common = ["-n", NS, "-r", 24000, "-b", 64, "-t", 1712345678, "--feed", mp2, "--feed-bitrate", 192, "--feed-rate", 48000, "--feed-drop-every", EVERY, "--feed-drop-run", RUN]
    r = run([exe, "-", tmp_path / "don.af"] + common + ["--conceal"])
    assert line("editick", NS, 16) in r.stderr, r.stderr
    run([exe, "-", tmp_path / "doff.af"] + common)
    on, off = af_packets(tmp_path / "don.af"), af_packets(tmp_path / "doff.af")
    assert len(on) == len(off) >= 8 and on != off
    bad = subprocess.run(["timeout", "-k", "10", "60", str(exe), str(mp2), str(tmp_path / "x.af"), "--conceal"], capture_output=True, text=True)
    assert bad.returncode == 1 and "strict --feed" in bad.stderr  # no feed: refused before anything runs, with the message it had


def test_nodetick_and_mp2enc_take_the_option(tmp_path, sources):
    exe = build(tmp_path, "nodetick")
    mp2, frames = sources[32000]
    common = ["-n", NS, "-d", "0", "-k", 12, "--feed", mp2, "--feed-bitrate", 128, "--feed-rate", 32000, "--feed-drop-every", EVERY, "--feed-drop-run", RUN]
    r = run([exe, "-", "-o", tmp_path / "on.af"] + common + ["--conceal"])
    assert line("nodetick", NS, 8) in r.stderr, r.stderr         # twelve ticks at 3/2 want eight frames
    run([exe, "-", "-o", tmp_path / "off.af"] + common)
    assert af_packets(tmp_path / "on.af") != af_packets(tmp_path / "off.af")
    mp2d, _ = sources[48000]
    r = run([exe, "-", "-n", NS, "-d", "0", "-k", 8, "-r", 24000, "-b", 64, "--feed", mp2d, "--feed-bitrate", 192, "--feed-rate", 48000,
             "--feed-drop-every", EVERY, "--feed-drop-run", RUN, "--conceal"])
    assert line("nodetick", NS, 16) in r.stderr, r.stderr        # eight ticks at 1/2 want sixteen
    # mp2enc --from-mp2 -r 48000 --conceal on a 32 kHz file whose frames 3 and 4 have a damaged CRC-16
    hurt = [bytes(bytearray(b[:5]) + bytes([b[5] ^ 1]) + b[6:]) if f in (3, 4) else b for f, b in enumerate(frames)]
    (tmp_path / "hurt.mp2").write_bytes(b"".join(hurt))
    exe = build(tmp_path, "mp2enc")
    r = run([exe, tmp_path / "hurt.mp2", tmp_path / "a.mp2", "--from-mp2", "-r", 48000, "-b", 128, "--conceal"])
    assert "mp2enc: conceal: 16 slots, 14 passed, 2 concealed, 0 muted, 1 runs, longest 2" in r.stderr, r.stderr
    run([exe, tmp_path / "hurt.mp2", tmp_path / "b.mp2", "--from-mp2", "-r", 48000, "-b", 128])
    a, b = (tmp_path / "a.mp2").read_bytes(), (tmp_path / "b.mp2").read_bytes()
    assert len(a) == len(b) > 0 and a != b
