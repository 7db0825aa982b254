"""Down feeds (include/toolame_batch.h, tlb_feed_down_*): the schedule through tlb_feed_down_want_at against its closed form in Python ints
and against the anchors of the header, the legal pairs, and the export list.  Host arithmetic only: no GPU."""
import ctypes as C
import re

import pytest

import feeddownlib as A

N = 1152
PAIRS = [(48000, 1, 2, 1), (32000, 3, 4, 3), (44100, 80, 147, 80)]   # feed rate, L, M, period in ticks


@pytest.fixture(scope="module")
def lib():
    import odr_audioenc_amd as M
    if not M.LIB_PATH.exists():
        M.build()
    L = C.CDLL(str(M.LIB_PATH))
    L.tlb_feed_down_want_at.argtypes = [C.c_long, C.c_long, C.c_long]
    return L


def test_the_anchors(lib):
    w = lambda fs, n: [lib.tlb_feed_down_want_at(fs, 24000, f) for f in range(n)]
    assert w(48000, 12) == [2] * 12
    assert w(32000, 9) == [2, 1, 1] * 3
    one = [f for f, x in enumerate(w(44100, 80)) if x == 1]
    assert len(one) == 13 and one[:8] == [6, 12, 18, 24, 30, 36, 43, 49] and set(w(44100, 80)) == {1, 2}


@pytest.mark.parametrize("fs,L,Mm,period", PAIRS, ids=["1_2", "3_4", "80_147"])
def test_want_is_the_closed_form_over_400_ticks(lib, fs, L, Mm, period):
    got = [lib.tlb_feed_down_want_at(fs, 24000, f) for f in range(400)]
    assert got == [A.want(f, L, Mm) for f in range(400)] and set(got) <= {1, 2}
    assert sum(got[:period]) == {1: 2, 3: 4, 80: 147}[period] and got[period:2 * period] == got[:period]
    # a tick never needs a source frame that has not arrived, and what is unconsumed before a tick is bounded
    left = [A.K(f - 1, L, Mm) * N - A.S(f, L, Mm) for f in range(401)]          # unconsumed before tick f
    assert all(A.K(f, L, Mm) * N - A.S(f + 1, L, Mm) >= 0 for f in range(400))
    assert min(left) >= 0 and max(left) == {1: 0, 3: 768, 80: 1137}[period]
    assert [A.S(f + 1, L, Mm) - A.S(f, L, Mm) for f in range(10)] == [lib.tlb_decimate_need_at(fs, 24000, f) for f in range(10)]
    # far from the reset: the position is the tick modulo the period
    for f in (10 ** 6, 10 ** 9 + 7, 2 ** 31 + 5):
        assert lib.tlb_feed_down_want_at(fs, 24000, f) == A.want(f, L, Mm)
    assert lib.tlb_feed_down_want_at(fs, 24000, -1) == -18


def test_illegal_pairs(lib):
    import odr_audioenc_amd as M
    rates = (48000, 44100, 32000, 24000, 22050, 16000)
    legal = {(48000, 24000), (44100, 24000), (32000, 24000)}
    for fs in rates:
        for es in rates:
            n = lib.tlb_feed_down_want_at(fs, es, 0)
            assert (n in (1, 2)) if (fs, es) in legal else n == -1, (fs, es)      # TLB_ERR_SAMPLERATE
            try:
                M.feed_want_at(fs, es, 0)
                assert (fs, es) not in legal                                      # every pair tlb_feed_want_at takes is illegal here
            except M.ToolameError:
                pass
    assert M.down_feed_want_at(44100, 24000, 6) == 1
    with pytest.raises(M.ToolameError):
        M.down_feed_want_at(48000, 48000, 0)


def test_every_declared_symbol_is_exported(lib):
    src = re.sub(r"/\*.*?\*/", " ", (A.ROOT / "include" / "toolame_batch.h").read_text(), flags=re.S)
    names = sorted(set(re.findall(r"\b(tlb_feed_down_[a-z0-9_]+)\s*\(", src)))
    assert {"tlb_feed_down_set", "tlb_feed_down_get", "tlb_feed_down_want", "tlb_feed_down_want_at", "tlb_feed_down_stride", "tlb_feed_down_reset",
            "tlb_feed_down_device", "tlb_feed_down_host"} <= set(names)
    for n in names:
        assert hasattr(lib, n), n
