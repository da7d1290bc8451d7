"""The segmented radix sort on its own (rdrf_selftest_sort_seg) against np.argsort(kind="stable") per segment.

nseg independent stable sorts of seg_len consecutive entries over the low `bits` bits; the bits above ride along; order holds
GLOBAL positions segment * seg_len + index.  Segment lengths at the 64-entry round, the wave-quarter (512) and the 2048-entry tile
edges (a tile must not straddle two segments); bits at the one-, two- and three-pass edges and with an uneven last digit.  Output
and temporary storage are filled with 0xFF before every call."""

import numpy as np
import pytest
import torch

from _util import pkg

pytestmark = pytest.mark.gpu

SEG_LENS = [1, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 3 * 2048 + 1]
BITS = [1, 8, 9, 10, 17, 18, 19]


def seg_sort(keys, nseg, seg_len, bits, count=None):
    """-> (keys_out, order, temp after the call) as uint32 / uint8 arrays; outputs pre-filled with 0xFF bytes"""
    L = pkg()
    n = nseg * seg_len
    assert len(keys) == n
    k = torch.from_numpy(keys.view(np.int32).copy()).cuda()
    ko = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    oo = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    tmp = torch.full((L.lib.rdrf_selftest_sort_seg_temp_bytes(nseg, seg_len, bits),), 0xFF, dtype=torch.uint8, device="cuda")
    cnt = None if count is None else torch.tensor([count], dtype=torch.int32, device="cuda")
    rc = L.lib.rdrf_selftest_sort_seg(L.ptr(k), nseg, seg_len, bits, L.ptr(cnt), L.ptr(ko), L.ptr(oo), L.ptr(tmp), tmp.numel(),
                                      L.stream_of(k))
    torch.cuda.synchronize()
    L.check(rc, "rdrf_selftest_sort_seg")
    assert torch.equal(k.cpu(), torch.from_numpy(keys.view(np.int32))), "the sort changed its input keys"
    return ko.cpu().numpy().view(np.uint32), oo.cpu().numpy().view(np.uint32)


def reference(keys, nseg, seg_len, bits):
    mask = np.uint32(0xffffffff if bits >= 32 else (1 << bits) - 1)
    ks, os_ = [], []
    for s in range(nseg):
        seg = keys[s * seg_len:(s + 1) * seg_len]
        o = np.argsort(seg & mask, kind="stable").astype(np.uint32)
        ks.append(seg[o])
        os_.append(o + np.uint32(s * seg_len))
    return np.concatenate(ks), np.concatenate(os_)


def patterns(n, bits, rng):
    top = (1 << bits) - 1
    above = rng.integers(0, 1 << (32 - bits), n, dtype=np.uint64) << np.uint64(bits)
    return {
        # one digit run as long as the tile: the order is the positions in ascending order, or the sort is not stable
        "equal": np.full(n, top // 3, dtype=np.uint64),
        # strictly descending as 32-bit keys (the sorted low bits wrap where n > 2^bits)
        "descending": (np.uint64(n - 1) - np.arange(n, dtype=np.uint64)) + np.uint64(5 << 24),
        # equal in the sorted bits, different above them: the upper bits must ride along untouched, in position order
        "above": above | np.uint64(top // 2),
        "random": rng.integers(0, 1 << 32, n, dtype=np.uint64),
    }


@pytest.mark.parametrize("seg_len", SEG_LENS)
def test_segments_sort_independently_stably_and_exactly(seg_len):
    rng = np.random.default_rng(seg_len)
    for nseg in (1, 3):
        n = nseg * seg_len
        for bits in BITS:
            for name, k in patterns(n, bits, rng).items():
                keys = k.astype(np.uint32)
                want_k, want_o = reference(keys, nseg, seg_len, bits)
                got_k, got_o = seg_sort(keys, nseg, seg_len, bits)
                where = f"seg_len {seg_len} nseg {nseg} bits {bits} {name}"
                assert np.array_equal(got_k, want_k), f"{where}: keys differ at {np.nonzero(got_k != want_k)[0][:4]}"
                assert np.array_equal(got_o, want_o), f"{where}: not stable at {np.nonzero(got_o != want_o)[0][:4]}"


@pytest.mark.parametrize("count", [0, 1, 2048, 2049])
def test_a_device_count_sets_length_and_stride_and_the_rest_is_left_alone(count):
    """launches sized for 3 segments of 3 * 2048 + 1; the segments are *count entries long and *count apart"""
    nseg, seg_len = 3, 3 * 2048 + 1
    rng = np.random.default_rng(count)
    for bits in (8, 17, 19):
        keys = rng.integers(0, 1 << 32, nseg * seg_len, dtype=np.uint64).astype(np.uint32)
        want_k, want_o = reference(keys[:nseg * count], nseg, count, bits)
        got_k, got_o = seg_sort(keys, nseg, seg_len, bits, count)
        m = nseg * count
        assert np.array_equal(got_k[:m], want_k) and np.array_equal(got_o[:m], want_o), f"count {count} bits {bits}"
        assert (got_k[m:] == 0xffffffff).all() and (got_o[m:] == 0xffffffff).all(), f"count {count} bits {bits}: wrote beyond 3 * count"


@pytest.mark.parametrize("kb", [15, 17])
@pytest.mark.parametrize("seg_len", [2049, 3 * 2048 + 1])
def test_three_segments_over_kb_bits_equal_one_sort_over_kb_plus_two(kb, seg_len):
    """keys as the key kernel of the sorted scatter builds them: segment p carries p << kb above its cell bits"""
    L = pkg()
    rng = np.random.default_rng(kb * seg_len)
    n = 3 * seg_len
    cell = rng.integers(0, 1 << kb, n, dtype=np.uint64)
    cell[rng.random(n) < 0.3] = (1 << kb) - 1                      # dropped keys
    keys = ((np.repeat(np.arange(3, dtype=np.uint64), seg_len) << np.uint64(kb)) | cell).astype(np.uint32)
    got_k, got_o = seg_sort(keys, 3, seg_len, kb)
    k = torch.from_numpy(keys.view(np.int32).copy()).cuda()
    ko = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    oo = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    tmp = torch.full((L.lib.rdrf_selftest_sort_temp_bytes(n, kb + 2),), 0xFF, dtype=torch.uint8, device="cuda")
    rc = L.lib.rdrf_selftest_sort(L.ptr(k), n, kb + 2, None, 0, L.ptr(ko), L.ptr(oo), L.ptr(tmp), tmp.numel(), L.stream_of(k))
    torch.cuda.synchronize()
    L.check(rc, "rdrf_selftest_sort")
    assert got_k.tobytes() == ko.cpu().numpy().tobytes() and got_o.tobytes() == oo.cpu().numpy().tobytes()
    want_k, want_o = reference(keys, 1, n, kb + 2)
    assert np.array_equal(got_k, want_k) and np.array_equal(got_o, want_o)


def test_bad_arguments_are_refused():
    L = pkg()
    k = torch.zeros(64, dtype=torch.int32, device="cuda")
    tmp = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    st = L.stream_of(k)
    assert L.lib.rdrf_selftest_sort_seg(L.ptr(k), 3, 8, 0, None, L.ptr(k), L.ptr(k), L.ptr(tmp), tmp.numel(), st) == -1
    assert L.lib.rdrf_selftest_sort_seg(L.ptr(k), 0, 8, 9, None, L.ptr(k), L.ptr(k), L.ptr(tmp), tmp.numel(), st) == -1
    assert L.lib.rdrf_selftest_sort_seg(L.ptr(k), 3, 8, 9, None, L.ptr(k), L.ptr(k), L.ptr(tmp), 16, st) == -3
    assert L.lib.rdrf_selftest_sort_seg(None, 3, 0, 9, None, None, None, None, 0, st) == 0
