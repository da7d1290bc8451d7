"""The radix sort's pass / digit plan and temporary-storage formula (rdrf_selftest_sort_describe, host code only).  No GPU.

The sorted scatter sorts the three planes' keys as three segments over the kb cell bits alone: kb = 15 (stage 0) must take two
passes of 8 bits, kb = 17 (final stage) two passes of 9, kb = 19 three passes; the segmented temp-size formula must cover what the
sort carves out of its temporary storage at every shape the GPU tests use."""
import ctypes as C

import pytest

from _util import pkg

SEG_LENS = [1, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 3 * 2048 + 1]
BITS = [1, 8, 9, 10, 17, 18, 19]
TILE = 2048


def describe(nseg, seg_len, bits):
    L = pkg()
    out = (C.c_ulonglong * 16)()
    n = L.lib.rdrf_selftest_sort_describe(nseg, seg_len, bits, out, 16)
    assert n == 9 and out[0] == 9, L.lib.rdrf_last_error()
    keys = ("passes", "digit_bits", "tiles_per_segment", "tile", "carved", "temp_bytes", "sort_launches", "call_launches")
    return dict(zip(keys, (int(v) for v in out[1:9])))


def test_symbols_are_bound():
    L = pkg()
    for s in ("rdrf_selftest_sort_seg_temp_bytes", "rdrf_selftest_sort_seg", "rdrf_selftest_sort_describe"):
        assert s in L.SYMBOLS and hasattr(L.lib, s)


@pytest.mark.parametrize("kb,passes,digit", [(15, 2, 8), (17, 2, 9), (19, 3, 7), (18, 2, 9), (9, 1, 9), (10, 2, 5), (1, 1, 1), (8, 1, 8)])
def test_pass_and_digit_plan(kb, passes, digit):
    d = describe(3, 4096 * 115, kb)
    assert (d["passes"], d["digit_bits"]) == (passes, digit)
    assert d["passes"] * d["digit_bits"] >= kb and d["digit_bits"] <= 9
    # a pass is histogram + scan + scatter; the key kernel of a sorted-scatter call takes the first histogram's place
    assert d["sort_launches"] == 3 * passes and d["call_launches"] == 1 + 3 * passes - 1


def test_the_sorted_bits_alone_save_the_final_stage_a_pass():
    """kb + 2 bits (plane bits sorted too) against kb bits: 19 -> 17 drops the third pass, 17 -> 15 halves the bins"""
    assert describe(1, 4096, 19)["passes"] == 3 and describe(3, 4096, 17)["passes"] == 2
    assert describe(1, 4096, 17)["digit_bits"] == 9 and describe(3, 4096, 15)["digit_bits"] == 8


@pytest.mark.parametrize("nseg", [1, 3])
def test_temp_formula_covers_the_carver(nseg):
    L = pkg()
    for seg_len in SEG_LENS + [0, 4096 * 115, 4096 * 345]:
        for bits in BITS + [32]:
            d = describe(nseg, seg_len, bits)
            assert d["tile"] == TILE and d["tiles_per_segment"] == (seg_len + TILE - 1) // TILE
            assert d["temp_bytes"] == L.lib.rdrf_selftest_sort_seg_temp_bytes(nseg, seg_len, bits)
            assert d["carved"] <= d["temp_bytes"], (nseg, seg_len, bits, d)
            # two key-sized arrays + per (segment, tile) 512 bins and a drop count + per segment the 512 totals
            tiles = max(1, d["tiles_per_segment"])
            assert d["carved"] >= 2 * nseg * seg_len * 4 + nseg * tiles * (512 + 1) * 4 + nseg * 512 * 4
            if nseg == 1:   # the one-segment entry point reports the same storage
                assert L.lib.rdrf_selftest_sort_temp_bytes(seg_len, bits) == d["temp_bytes"]


def test_describe_rejects_bad_arguments():
    L = pkg()
    out = (C.c_ulonglong * 16)()
    assert L.lib.rdrf_selftest_sort_describe(3, 100, 0, out, 16) == -1
    assert L.lib.rdrf_selftest_sort_describe(0, 100, 9, out, 16) == -1
    assert L.lib.rdrf_selftest_sort_describe(3, 100, 9, out, 4) == -3
    assert L.lib.rdrf_selftest_sort_describe(3, 100, 9, None, 16) == -3
