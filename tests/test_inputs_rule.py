"""Which input families may stand beside one another (csrc/tlb_inputs.h), CPU only: the header every setter of the batch, the tick plane and
the node level asks.  tests/emu/inputs_main.cpp prints the header's answer for every (present mask, family to set) pair under AddressSanitizer
and UBSan; the two relations are written out here once more, literally, and every answer is compared.  The program is linked with the
sanitizers; nothing is preloaded."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent

UP, DOWN, FEED, DOWN_FEED, SHORT = range(5)      # the enum's order
# one stream of a batch: a stream has one source, but a feed's PCM may still pass the resampler or the decimator
STREAM_CLASHES = {frozenset(p) for p in [(DOWN_FEED, FEED), (DOWN_FEED, UP), (DOWN_FEED, DOWN), (UP, DOWN)]}
# one tick or node object: all five exclude one another
OBJECT_CLASHES = {frozenset((a, b)) for a in range(5) for b in range(5) if a != b}


def expected(clashes, families):
    return {(present, f): int(not any(present >> g & 1 and frozenset((f, g)) in clashes for g in range(families)))
            for present in range(1 << families) for f in range(families)}


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")
def test_every_answer_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "inputs_main"
    src = ROOT / "tests" / "emu" / "inputs_main.cpp"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    lines = r.stdout.split("\n")
    assert lines[-2] == "inputs ok: %d answers" % (16 * 4 + 32 * 5)
    got = [{}, {}]
    for line in lines[:-2]:
        level, present, f, answer = map(int, line.split())
        got[level][(present, f)] = answer
    assert got[0] == expected(STREAM_CLASHES, 4)
    assert got[1] == expected(OBJECT_CLASHES, 5)
    # symmetry: with only g present f may be set exactly when, with only f present, g may be set; and no family excludes itself
    for answers, families in ((got[0], 4), (got[1], 5)):
        for f in range(families):
            assert answers[(1 << f, f)] == 1
            for g in range(families):
                assert answers[(1 << g, f)] == answers[(1 << f, g)]
    # the pairs that stay legal on a batch stream
    assert got[0][(1 << UP, FEED)] == got[0][(1 << FEED, UP)] == got[0][(1 << DOWN, FEED)] == got[0][(1 << FEED, DOWN)] == 1
