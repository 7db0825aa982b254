"""Layer II feeds, the host-only part of the C-ABI (no GPU): tlb_feed_check_config and tlb_feed_frame_bytes over every (sample rate,
bitrate, channels) cell, legal and illegal, against the table of tests/sweeplib.py (every configuration the oracle encoder accepts, found
by trying); and the symbols the library exports."""
import ctypes as C

import pytest

import declib as D
import sweeplib as S

FEED_SYMS = ["tlb_feed_check_config", "tlb_feed_frame_bytes", "tlb_feed_set", "tlb_feed_get", "tlb_feed_stride", "tlb_feed_reset",
             "tlb_feed_device", "tlb_feed_host"]
OK, ERR_SAMPLERATE, ERR_MODE, ERR_BITRATE = 0, 1, 2, 4


@pytest.fixture(scope="module")
def M():
    import odr_audioenc_amd as M
    if not M.LIB_PATH.exists():
        M.build()
    return M


def test_symbols_are_exported(M):
    lib = C.CDLL(str(M.LIB_PATH))
    for name in FEED_SYMS:
        assert hasattr(lib, name), name


def test_check_config_and_frame_bytes_over_every_cell(M):
    """a (rate, bitrate, channels) cell is legal exactly when sweeplib's table has the rate with that bitrate for a mode of that channel
    count: 'm' for one channel, 's' / 'j' / 'd' for two"""
    legal = S.legal_configs()
    table = {1: {(fs, kbps) for fs, mode, kbps in legal if mode == "m"}, 2: {(fs, kbps) for fs, mode, kbps in legal if mode != "m"}}
    for ch in (1, 2):                                            # the two-channel modes agree among themselves
        assert all({(fs, kbps) for fs, mode, kbps in legal if mode == m} == table[2] for m in "sjd")
    rates = list(S.RATES) + [8000, 11025, 12000, 96000, 0, -48000]
    cells = n_legal = 0
    for fs in rates:
        for kbps in list(range(-8, 457, 8)) + [1, 100, 129]:
            for ch in (0, 1, 2, 3):
                cfg = M.FeedConfig(fs, kbps, ch)
                rc = M.feed_check_config(cfg)
                cells += 1
                if ch in (1, 2) and (fs, kbps) in table[ch]:
                    n_legal += 1
                    assert rc == OK, (fs, kbps, ch, rc)
                    assert M.feed_frame_bytes(cfg) == D.frame_bytes_of(dict(samplerate=fs, kbps=kbps)), (fs, kbps, ch)
                else:
                    want = ERR_MODE if ch not in (1, 2) else ERR_BITRATE if (kbps <= 0 or fs in S.RATES) else ERR_SAMPLERATE
                    assert rc == want, (fs, kbps, ch, rc, want)
                    with pytest.raises(M.ToolameError) as e:
                        M.feed_frame_bytes(cfg)
                    assert e.value.code == want
    assert n_legal == len(table[1]) + len(table[2]) == 2 * 6 * 14 and cells > 2500


def test_null_config_is_an_argument_error(M):
    lib = M.load_library()
    assert lib.tlb_feed_check_config(None) == 18 and lib.tlb_feed_frame_bytes(None) == -18
    assert lib.tlb_feed_set(None, 0, None) == 18 and lib.tlb_feed_stride(None) == 0 and lib.tlb_feed_reset(None, 0) == 18
    assert lib.tlb_feed_get(None, 0, None) == -18
    assert lib.tlb_feed_host(None, None, None, 1, None, None) == 18 and lib.tlb_feed_device(None, None, None, 1, None, None, None) == 18
