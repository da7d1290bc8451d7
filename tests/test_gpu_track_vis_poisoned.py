"""rdrf_track_visibility_fwd on hostile scratch (the style of test_gpu_poisoned_scratch.py): the output buffer and the workspace
are filled with 0xFF bytes (a NaN in every float, -1 in every list entry and counter) before the call, with guard bands around
both.  Every visibility is finite and has the bits of the run on fresh buffers; the guards stay untouched.  The kernels may
read only what the call itself wrote: the list counter is cleared by the time-branch launch, sigma and blending of every sample
that no density kernel visits are zero-filled by the keep pass."""

import pytest
import torch

import test_gpu_track_vis as V

from _twin import same_bits
from _util import pkg

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("packed", [True, False], ids=["packed-image", "packs-into-workspace"])
@pytest.mark.parametrize("rt,M,S", [("ndc", 33, 65), ("contract", 70, 13)])
def test_poisoned_output_and_workspace(rt, M, S, packed, monkeypatch):
    R = pkg("renderer")
    F = pkg("fields")
    L = pkg()
    monkeypatch.setattr(F, "PACK_CACHE", packed)
    _, st, dy, _, _, focal, H, W = V.scene(rt)
    n_fwd, n_bwd, K, G = 5, 3, 9, 257
    tr, t0, cams = V.tracks_of(rt, M, n_fwd, n_bwd)
    margin = 2.0 * V.step_of(rt, S)
    dt = 2.0 / (V.T_VIDEO - 1)
    ref = R._track_visibility_raw(st, dy, tr.points, t0, n_fwd, n_bwd, dt, cams, focal, H, W, S, rt, margin)
    assert bool(torch.isfinite(ref).all())
    big = torch.full((G + M * K + G,), float("nan"), device=V.DEV)
    big.view(torch.uint8).fill_(0xFF)
    vis = big[G:G + M * K].view(M, K)
    nbytes = int(L.lib.rdrf_track_visibility_ws_bytes(M, K, S))
    assert nbytes % 4 == 0
    ws = torch.full((nbytes + 4 * G,), 0xFF, dtype=torch.uint8, device=V.DEV)
    R._track_visibility_raw(st, dy, tr.points, t0, n_fwd, n_bwd, dt, cams, focal, H, W, S, rt, margin, vis=vis, ws=ws[:nbytes])
    torch.cuda.synchronize()
    assert bool(torch.isfinite(vis).all())
    assert same_bits(vis.contiguous(), ref)
    assert bool((big[:G].view(torch.uint8) == 0xFF).all()) and bool((big[G + M * K:].view(torch.uint8) == 0xFF).all())
    assert bool((ws[nbytes:] == 0xFF).all())
