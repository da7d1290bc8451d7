"""rdrf_render_hits_fwd on hostile scratch (the style of test_gpu_track_vis_poisoned.py): the hit buffers, the map buffers and
the workspace are filled with 0xFF bytes (a NaN in every float, -1 in every list entry and counter) before the call, with guard
bands around the outputs and behind the workspace.  Every requested output is fully written and has the bits of the run on
fresh buffers, on the render path and on the density-only path, with the packed weight images and with images packed into the
workspace; the guards stay untouched.  The kernels may read only what the call itself wrote."""

import pytest
import torch

import test_gpu_hits as T
import test_gpu_track_vis as V

from _twin import same_bits
from _util import pkg

pytestmark = pytest.mark.gpu
G = 257


def _poisoned(shape, dtype):
    n = 1
    for d in shape:
        n *= d
    big = torch.empty(G + n + G, dtype=dtype, device=V.DEV)
    big.view(torch.uint8).fill_(0xFF)
    return big, big[G:G + n].view(shape)


@pytest.mark.parametrize("packed", [True, False], ids=["packed-image", "packs-into-workspace"])
@pytest.mark.parametrize("maps", [False, True], ids=["density-only", "render"])
@pytest.mark.parametrize("rt,S", [("ndc", 65), ("contract", 13)])
def test_poisoned_outputs_and_workspace(rt, S, maps, packed, monkeypatch):
    R = pkg("renderer")
    F = pkg("fields")
    L = pkg()
    monkeypatch.setattr(F, "PACK_CACHE", packed)
    _, st, dy = V.scene(rt)[:3]
    rays, ts = T.batch(rt)
    N, taus = rays.shape[0], list(T.T8)
    names = L.RENDER_MAPS if maps else ()
    ref, mref = R._render_hits_raw(st, dy, rays, ts, taus, S, rt, names)
    torch.cuda.synchronize()
    shapes = {"z": (8, N), "hit": (8, N), "xyz": (8, N, 3), "owner": (8, N)}
    bigs, bufs = {}, {}
    for n, shp in shapes.items():
        bigs[n], bufs[n] = _poisoned(shp, torch.uint8 if n == "hit" else torch.float32)
    mbufs = {}
    for n in names:
        bigs["map." + n], mbufs[n] = _poisoned((N, 3) if n.startswith("rgb") else (N,), torch.float32)
    nbytes = int(L.lib.rdrf_render_hits_ws_bytes(N, S))
    ws = torch.full((nbytes + 4 * G,), 0xFF, dtype=torch.uint8, device=V.DEV)
    R._render_hits_raw(st, dy, rays, ts, taus, S, rt, names, bufs=bufs, mbufs=mbufs, ws=ws[:nbytes])
    torch.cuda.synchronize()
    for n in shapes:
        assert same_bits(bufs[n].contiguous(), ref[n]), n
    assert bool((bufs["hit"] <= 1).all()) and bool(torch.isfinite(bufs["z"]).all()) and bool(torch.isfinite(bufs["xyz"]).all())
    for n in names:
        assert same_bits(mbufs[n].contiguous(), mref[n]), n
    for n, big in bigs.items():
        flat = big.view(torch.uint8)
        g = G * big.element_size()
        assert bool((flat[:g] == 0xFF).all()) and bool((flat[-g:] == 0xFF).all()), n
    assert bool((ws[nbytes:] == 0xFF).all())
