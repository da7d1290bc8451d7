"""Rows are saved only where a backward can read them: the host-side decisions, checked without a GPU."""
import types

import pytest
import torch

from _util import pkg


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_alloc_saved_follows_the_grad_mode(kind):
    """ctx.needs_input_grad reports True for parameters under torch.no_grad() too (no backward can exist there), so
    _alloc_saved looks at the grad mode: None under no_grad, a buffer of rdrf_saved_bytes otherwise; the mode the field
    modules captured from their caller (inside Function.forward grad mode is always off) overrides the ambient one."""
    F, L = pkg("fields"), pkg()
    ctx = types.SimpleNamespace(needs_input_grad=(True,) * 8)
    N, S = 70, 13
    with torch.no_grad():
        assert F._alloc_saved(ctx, kind, N, S, "cpu") == (None, 0)
        buf, n = F._alloc_saved(ctx, kind, N, S, "cpu", True)
        assert buf is not None and n == buf.numel() == L.lib.rdrf_saved_bytes(kind, N, S)
    buf, n = F._alloc_saved(ctx, kind, N, S, "cpu")
    assert buf is not None and buf.dtype == torch.uint8 and n == buf.numel() == L.lib.rdrf_saved_bytes(kind, N, S)
    assert F._alloc_saved(ctx, kind, N, S, "cpu", False) == (None, 0)
    none = types.SimpleNamespace(needs_input_grad=(False,) * 8)
    assert F._alloc_saved(none, kind, N, S, "cpu") == (None, 0)


@pytest.mark.parametrize("dynamic", [0, 1])
def test_feat_saved_follows_the_grad_mode(dynamic):
    F, L = pkg("fields"), pkg()
    ctx = types.SimpleNamespace(needs_input_grad=(True,) * 8)
    with torch.no_grad():
        assert F._feat_saved(ctx, dynamic, 70, "cpu") == (None, 0)
    buf, n = F._feat_saved(ctx, dynamic, 70, "cpu")
    assert n == buf.numel() == L.lib.rdrf_features_saved_bytes(dynamic, 70)


@pytest.mark.parametrize("N,S", [(70, 13), (70, 45), (1, 1), (4096, 115)])
def test_no_app_buffer_is_the_full_one_minus_the_appearance_block(N, S):
    """rdrf_saved_bytes_ex(RDRF_SAVE_NO_APP): the layout without its last block -- ceil(N S / 32) tiles of
    rdrf_saved_row_bytes(appearance phase) x 32 samples, padded to 256 bytes like every block; flags = 0 is the plain size,
    the scene-flow buffer (kind 2) has no appearance rows to drop."""
    F, L = pkg("fields"), pkg()
    tiles = (N * S + 31) // 32
    for kind, phase in ((0, 2), (1, 1)):
        full = L.lib.rdrf_saved_bytes(kind, N, S)
        assert L.lib.rdrf_saved_bytes_ex(kind, N, S, 0) == full
        block = tiles * 32 * L.lib.rdrf_saved_row_bytes(phase) + 256
        assert block % 256 == 0
        assert L.lib.rdrf_saved_bytes_ex(kind, N, S, L.SAVE_NO_APP) == full - block
    assert L.lib.rdrf_saved_bytes_ex(2, N, S, L.SAVE_NO_APP) == L.lib.rdrf_saved_bytes(2, N, S)


def test_call_mode_round_trip():
    """the (rgb mode, grad mode) pair the field modules hand to their autograd Function as arguments of their own: the
    rgb mode as given, the grad mode of the caller"""
    F = pkg("fields")
    for rgb in (True, False, "value"):
        assert F._call_modes(rgb) == (rgb, True) and F._call_modes(rgb)[0] is rgb
        with torch.no_grad():
            assert F._call_modes(rgb) == (rgb, False) and F._call_modes(rgb)[0] is rgb
    with pytest.raises(ValueError):
        F._call_modes("values")
