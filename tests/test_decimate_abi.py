"""The decimator's C-ABI without a GPU: the names are declared and exported, tlb_decimate_need_at's arithmetic, NULL handles."""
import re
from pathlib import Path

import pytest

import decimatelib as D

ROOT = Path(__file__).resolve().parent.parent
NAMES = ["tlb_decimate_set_source", "tlb_decimate_source", "tlb_decimate_need", "tlb_decimate_need_at", "tlb_decimate_taps", "tlb_decimate_device",
         "tlb_decimate_host", "tlb_tick_set_down_source", "tlb_tick_down", "tlb_tick_down_need", "tlb_node_set_down_source", "tlb_node_down",
         "tlb_node_down_need"]
ERR_SAMPLERATE, ERR_ARG = 1, 18


def lib():
    import odr_audioenc_amd as M
    if not M.LIB_PATH.exists():
        M.build()
    return M.load_library()


def test_names_are_declared_and_exported():
    src = re.sub(r"/\*.*?\*/", " ", (ROOT / "include" / "toolame_batch.h").read_text(), flags=re.S)
    L = lib()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, src), n
        assert hasattr(L, n), n
    assert re.search(r"#define\s+TLB_DECIMATE_TAPS\s+64\b", src) and re.search(r"#define\s+TLB_DECIMATE_SLOT\s+4608\b", src)


@pytest.mark.parametrize("source,want", [(48000, {2304}), (32000, {1536}), (44100, {2116, 2117})])
def test_need_at_is_the_definition(source, want):
    import odr_audioenc_amd as M
    got = [M.decimate_need_at(source, 24000, f) for f in range(40)]
    assert set(got) == want
    assert got == [D.need(source, 24000, f) for f in range(40)]          # the header's formula in Python ints
    assert max(got) <= 2304                                              # a wide slot holds it
    if source == 44100:
        assert got[:5] == [2117, 2117, 2117, 2117, 2116] and got[:5] == got[5:10]
        for f in range(35):
            assert sum(got[f:f + 5]) == 10584
    assert M.decimate_need_at(source, 24000, 10 ** 9 + 3) == got[3]


def test_unsupported_pairs():
    L = lib()
    for pair in ((44100, 48000), (22050, 24000), (32000, 48000), (16000, 24000), (48000, 48000), (24000, 24000), (48000, 44100), (48000, 32000), (96000, 24000)):
        assert L.tlb_decimate_need_at(pair[0], pair[1], 0) == -ERR_SAMPLERATE, pair
    assert L.tlb_decimate_need_at(48000, 24000, -1) == -ERR_ARG
    assert L.tlb_resample_need_at(48000, 24000, 0) == -ERR_SAMPLERATE    # the resampler has not learnt the pair


def test_null_handles():
    L = lib()
    assert L.tlb_decimate_set_source(None, 0, 48000) == ERR_ARG
    assert L.tlb_decimate_source(None, 0) == 0
    assert L.tlb_decimate_need(None, 0, 0) == -ERR_ARG
    assert L.tlb_decimate_device(None, None, 1, None, None) == ERR_ARG
    assert L.tlb_decimate_host(None, None, 1, None) == ERR_ARG
    assert L.tlb_tick_set_down_source(None, 0, 48000) == ERR_ARG
    assert L.tlb_tick_down_need(None, 0) == -ERR_ARG
    assert not L.tlb_tick_down(None, 0)
    assert L.tlb_node_set_down_source(None, 0, 48000) == ERR_ARG
    assert L.tlb_node_down_need(None, 0) == -ERR_ARG
    assert not L.tlb_node_down(None, 0)
    assert L.tlb_decimate_taps(48000, 24000, None, None, None)
    assert not L.tlb_decimate_taps(48000, 48000, None, None, None)
