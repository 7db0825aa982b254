"""Adapted feeds, the host-only part of the C-ABI (include/toolame_batch.h, tlb_feed_want_at): the schedule against its closed form in
Python ints, the anchors the header states, the illegal pairs and argument errors, and the new symbols in the dynamic symbol table.  No GPU."""
import subprocess

import pytest

import feedadaptlib as A
import odr_audioenc_amd as M

PAIRS = [(44100, 48000, 160, 147), (22050, 24000, 160, 147), (32000, 48000, 3, 2), (16000, 24000, 3, 2)]
EQUAL = [48000, 44100, 32000, 24000, 22050, 16000]


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not M.LIB_PATH.exists():
        M.build()


@pytest.mark.parametrize("fs,es,L,Mm", PAIRS)
def test_want_at_equals_the_closed_form_over_two_periods(fs, es, L, Mm):
    period = 160 if L == 160 else 3
    got = [M.feed_want_at(fs, es, t) for t in range(2 * period + 5)]
    assert got == [A.want(t, L, Mm) for t in range(2 * period + 5)]
    assert got[:period] == got[period:2 * period]
    assert M.feed_want_at(fs, es, 10 ** 9 + 7) == A.want((10 ** 9 + 7) % period, L, Mm)      # far from the reset: the period, not an overflow


@pytest.mark.parametrize("rate", EQUAL)
def test_equal_rates_want_every_tick(rate):
    assert [M.feed_want_at(rate, rate, t) for t in range(330)] == [1] * 330 == [A.want(t, 1, 1) for t in range(330)]


def test_the_anchors_of_the_definition():
    for L, Mm, period, wanted, bound in ((160, 147, 160, 147, 1145), (3, 2, 3, 2, 768), (1, 1, 1, 1, 0)):
        w = [A.want(f, L, Mm) for f in range(4 * period + 2)]
        assert set(w) <= {0, 1} and all(w[f] + w[f + 1] >= 1 for f in range(len(w) - 1))        # 0 or 1, never 0 on two consecutive ticks
        assert sum(w[:period]) == wanted and w[:period] == w[period:2 * period]
        # before any tick the unconsumed decoded source frames K(f - 1) 1152 - S(f), and the bound is reached
        left = [A.K(f - 1, L, Mm) * A.N - A.S(f, L, Mm) for f in range(4 * period + 2)]
        assert min(left) >= 0 and max(left) == bound
        for f in range(4 * period):
            assert A.S(f + 1, L, Mm) - A.S(f, L, Mm) == (M.resample_need_at({160: 44100, 3: 32000}[L], 48000, f) if L != 1 else A.N)
            # a tick's output touches [S(f) - 31, S(f + 1)): at most two feed frames, the older delivered at most two ticks earlier
            lo, hi = max(A.S(f, L, Mm) - 31, 0) // A.N, (A.S(f + 1, L, Mm) - 1) // A.N
            assert hi - lo <= 1 and hi < A.K(f, L, Mm)
            assert A.K(f - 3, L, Mm) <= lo                         # (frame `lo` had not arrived by tick f - 3)
    assert [f for f in range(60) if not A.want(f, 160, 147)] == [12, 24, 36, 49]
    assert [f for f in range(12) if not A.want(f, 3, 2)] == [2, 5, 8, 11]
    assert [f for f in range(60) if not M.feed_want_at(44100, 48000, f)] == [12, 24, 36, 49]
    assert [f for f in range(12) if not M.feed_want_at(16000, 24000, f)] == [2, 5, 8, 11]


@pytest.mark.parametrize("fs,es", [(48000, 24000), (44100, 24000), (8000, 48000), (48000, 44100), (0, 48000)])
def test_illegal_pairs(fs, es):
    L = M.load_library()
    assert L.tlb_feed_want_at(fs, es, 0) == -1                       # -TLB_ERR_SAMPLERATE
    with pytest.raises(M.ToolameError) as e:
        M.feed_want_at(fs, es, 0)
    assert e.value.code == 1


def test_argument_errors():
    L = M.load_library()
    assert L.tlb_feed_want_at(44100, 48000, -1) == -18
    assert L.tlb_feed_want_at(48000, 48000, -5) == -18
    assert L.tlb_feed_adapted(None, 0) == -18 and L.tlb_feed_want(None, 0, 0) == -18
    assert L.tlb_feed_set_adapted(None, 0, None) == 18
    assert L.tlb_tick_set_feed_adapted(None, 0, None) == 18 and L.tlb_tick_feed_want(None, 0) == -18
    assert L.tlb_node_set_feed_adapted(None, 0, None) == 18 and L.tlb_node_feed_want(None, 0) == -18


def test_the_new_symbols_are_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", str(M.LIB_PATH)], check=True, capture_output=True, text=True).stdout
    have = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for sym in ("tlb_feed_set_adapted", "tlb_feed_adapted", "tlb_feed_want", "tlb_feed_want_at", "tlb_tick_set_feed_adapted", "tlb_tick_feed_want",
                "tlb_node_set_feed_adapted", "tlb_node_feed_want"):
        assert sym in have, sym
    assert M.DEC_UNWANTED == 0x100 and not (M.DEC_UNWANTED & M.DEC_BAD_MASK)
