"""The carves fit what the size functions say.  Every *_workspace_bytes value the package asks for is the end offset of the carve
of the entry point that consumes it (csrc/rdrf_host.hpp, WsCarver in measuring mode), with no slack term behind it; _lib.workspace
hides that by rounding every request up by a quarter.  Here it hands out a view of exactly the requested bytes at the front of a
buffer that is 64 KiB longer, the tail filled with a canary byte, and forward + backward of both fields (ray and sorted scatter),
the scene flow and the per-point feature entry points run at the ragged shapes of test_gpu_poisoned_scratch: every call returns
0, every output and gradient is finite, and no canary byte changed.

Through the C ABI directly, the five backward entry points are then given a workspace 256 bytes (one carve block) short of what
they need: they return -3 and leave the gradient buffers, pre-filled with a marker, alone -- the carve stays the first thing
after the argument checks, ahead of the first launch.  rdrf_workspace_bytes is a maximum over several carves, so the need of
the entry point under test is measured: called with ws_bytes = 0 it reports "need <bytes> have 0" through rdrf_last_error.  That
need is no larger than the size function's value, and given exactly that many bytes the call succeeds without touching the
canary behind them."""
import contextlib
import ctypes as C
import re

import pytest
import torch

import test_gpu_poisoned_scratch as PS
from test_gpu_poisoned_scratch import M, N, S

from _util import pkg

pytestmark = pytest.mark.gpu

TAIL, CANARY, SENT = 64 << 10, 0xA5, 7.0


@contextlib.contextmanager
def exact_workspaces():
    L = pkg()
    orig, handed = L.workspace, []

    def exact(device, nbytes):
        nbytes = int(nbytes)
        buf = torch.full((nbytes + TAIL,), CANARY, dtype=torch.uint8, device=device)
        handed.append((buf, nbytes))
        return buf[:nbytes]

    L.workspace = exact
    try:
        yield handed
    finally:
        L.workspace = orig


def _canaries_intact(handed, what):
    torch.cuda.synchronize()
    bad = [(i, n) for i, (buf, n) in enumerate(handed) if not bool((buf[n:] == CANARY).all())]
    assert not bad, f"{what}: written past the requested workspace bytes (call index, bytes requested): {bad}"


@pytest.mark.parametrize("mode", ["ray", "sorted"])
def test_fields_and_scene_flow_stay_inside_the_requested_workspace(mode):
    st, dy = PS._fields("ndc")
    batch = PS._batch(dy, "ndc")
    with exact_workspaces() as handed:
        res = PS.run_rays(st, dy, batch, "ndc", mode, "full", True)      # (L.check raises on a non-zero return code)
    assert len(handed) >= 6, len(handed)      # forward + backward of both fields and of the scene flow
    PS._finite(res, f"exact workspace, {mode} scatter")
    assert any(k.startswith("grad.st.") for k in res) and any(k.startswith("grad.dy.") for k in res)
    _canaries_intact(handed, f"{mode} scatter")


def test_feature_entry_points_stay_inside_the_requested_workspace():
    st, dy = PS._fields("ndc")
    with exact_workspaces() as handed:
        res = PS.run_features(st, dy)
    assert len(handed) >= 4, len(handed)
    PS._finite(res, f"exact workspace, features M = {M}")
    assert any(k.startswith("grad.st.") for k in res) and any(k.startswith("grad.dy.") for k in res)
    _canaries_intact(handed, "features")


def _short_case(name):
    """-> (backward(ws, ws_bytes) -> rc, gradient tensors pre-filled with SENT, size function value) after the forward call that
    fills the saved buffer; everything the calls point to is kept alive by the closure"""
    L, F = pkg(), pkg("fields")
    st, dy = PS._fields("ndc")
    rays, ts, xyz, z, valid, _ = PS._batch(dy, "ndc")
    rays, ts, xyz, z = (L.f32c(t) for t in (rays, ts, xyz, z))
    valid8 = valid.contiguous().view(torch.uint8)
    dev = z.device
    dyn = "dynamic" in name or name == "rdrf_scene_flow_bwd"
    field = dy if dyn else st
    params = [p.detach() for p in field._param_list()]
    struct = F._dynamic_struct if dyn else F._static_struct
    grads = [torch.full_like(p, SENT) for p in params]
    P, G, cfg = struct(params), struct(grads), F._cfg_struct(field, "ndc")
    fws = torch.empty(max(int(L.lib.rdrf_workspace_bytes(N, S)), int(L.lib.rdrf_features_workspace_bytes(M))), dtype=torch.uint8, device=dev)
    ftail = (L.ptr(fws), C.c_size_t(fws.numel()), L.stream_of(z))
    new = lambda *shape: torch.empty(*shape, device=dev)
    ones = lambda *shape: torch.ones(*shape, device=dev)
    g = torch.Generator().manual_seed(12)
    xn = (torch.rand(M, 3, generator=g) * 1.9 - 0.95).cuda()
    tm = (torch.randint(0, 12, (M,), generator=g).float() * 2 / 11 - 1).cuda()
    keep = [params, grads, P, G, cfg, fws, rays, ts, xyz, z, valid8, xn, tm]
    if name in ("rdrf_static_bwd", "rdrf_dynamic_bwd"):
        head = (C.byref(P), C.byref(cfg), L.ptr(rays), L.ptr(ts), L.ptr(xyz), L.ptr(z), L.ptr(valid8), N, S)
        saved = torch.empty(int(L.lib.rdrf_saved_bytes(int(dyn), N, S)), dtype=torch.uint8, device=dev)
        stail = (L.ptr(saved), C.c_size_t(saved.numel()))
        outs = [new(N, S, 3), new(N, S), new(N, S), new(N, S), new(N, S), new(N, S, 3)]
        rgb, sigma, weight, dists, blending, xyz_prime = (L.ptr(o) for o in outs)
        if dyn:
            rc = L.lib.rdrf_dynamic_fwd(*head, blending, weight, xyz_prime, rgb, sigma, dists, *stail, *ftail)
        else:
            rc = L.lib.rdrf_static_fwd(*head, rgb, sigma, weight, dists, *stail, *ftail)
        gin = [torch.full_like(xyz, SENT), torch.full_like(z, SENT), torch.full_like(rays, SENT)]
        ups = [ones(N, S, 3), ones(N, S), ones(N, S), ones(N, S, 3)]
        g_rgb, g_sigma, g_blending, g_xyz_prime = (L.ptr(u) for u in ups)
        gtail = (C.byref(G), *(L.ptr(t) for t in gin), *stail)
        if dyn:   # g_blending, g_weight, g_xyz_prime, g_rgb, g_sigma, g_dists
            bwd = lambda ws, n: L.lib.rdrf_dynamic_bwd(*head, g_blending, None, g_xyz_prime, g_rgb, g_sigma, None, *gtail, L.ptr(ws),
                                                       C.c_size_t(n), L.stream_of(z))
        else:     # g_rgb, g_sigma, g_weight, g_dists
            bwd = lambda ws, n: L.lib.rdrf_static_bwd(*head, g_rgb, g_sigma, None, None, *gtail, L.ptr(ws), C.c_size_t(n), L.stream_of(z))
        size = int(L.lib.rdrf_workspace_bytes(N, S))
    elif name == "rdrf_scene_flow_bwd":
        head = (C.byref(P), C.byref(cfg), L.ptr(xyz), L.ptr(ts), N, S)
        saved = torch.empty(int(L.lib.rdrf_saved_bytes(2, N, S)), dtype=torch.uint8, device=dev)
        stail = (L.ptr(saved), C.c_size_t(saved.numel()))
        outs = [new(N, S, 3), new(N, S, 3)]
        rc = L.lib.rdrf_scene_flow_fwd(*head, L.ptr(outs[0]), L.ptr(outs[1]), *stail, *ftail)
        gin = [torch.full_like(xyz, SENT)]
        ups = [ones(N, S, 3), ones(N, S, 3)]
        bwd = lambda ws, n: L.lib.rdrf_scene_flow_bwd(*head, L.ptr(ups[0]), L.ptr(ups[1]), C.byref(G), L.ptr(gin[0]), *stail, L.ptr(ws),
                                                      C.c_size_t(n), L.stream_of(z))
        size = int(L.lib.rdrf_workspace_bytes(N, S))
    else:
        saved = torch.empty(int(L.lib.rdrf_features_saved_bytes(int(dyn), M)), dtype=torch.uint8, device=dev)
        stail = (L.ptr(saved), C.c_size_t(saved.numel()))
        outs = [new(M), new(M), new(M, 27), new(M, 3)]
        dens, blend, app, xp = (L.ptr(o) for o in outs)
        gin = [torch.full_like(xn, SENT)]
        ups = [ones(M), ones(M), ones(M, 27), ones(M, 3)]
        g_dens, g_blend, g_app, g_xp = (L.ptr(u) for u in ups)
        if dyn:
            head = (C.byref(P), C.byref(cfg), L.ptr(xn), L.ptr(tm), M, 1)
            rc = L.lib.rdrf_dynamic_features_fwd(*head, dens, blend, app, xp, *stail, *ftail)
            bwd = lambda ws, n: L.lib.rdrf_dynamic_features_bwd(*head, g_dens, g_blend, g_app, g_xp, C.byref(G), L.ptr(gin[0]), *stail,
                                                                L.ptr(ws), C.c_size_t(n), L.stream_of(z))
        else:
            head = (C.byref(P), C.byref(cfg), L.ptr(xn), M)
            rc = L.lib.rdrf_static_features_fwd(*head, dens, app, *stail, *ftail)
            bwd = lambda ws, n: L.lib.rdrf_static_features_bwd(*head, g_dens, g_app, C.byref(G), L.ptr(gin[0]), *stail, L.ptr(ws),
                                                               C.c_size_t(n), L.stream_of(z))
        size = int(L.lib.rdrf_features_bwd_workspace_bytes(M))
    L.check(rc, "forward of " + name)
    torch.cuda.synchronize()
    keep += [saved, outs, ups]

    def backward(ws, n):
        rc_ = bwd(ws, n)
        torch.cuda.synchronize()
        return rc_, L.lib.rdrf_last_error().decode(), keep

    return backward, grads + gin, size


@pytest.mark.parametrize("name", ["rdrf_static_bwd", "rdrf_dynamic_bwd", "rdrf_static_features_bwd", "rdrf_dynamic_features_bwd",
                                  "rdrf_scene_flow_bwd"])
def test_backward_refuses_a_workspace_one_block_short(name):
    backward, gouts, size = _short_case(name)
    untouched = lambda: all(bool((t == SENT).all()) for t in gouts)
    ws = torch.full((size + TAIL,), CANARY, dtype=torch.uint8, device="cuda")
    rc, msg, _ = backward(ws, 0)
    found = re.search(r"need (\d+) have 0\b", msg)
    assert rc == -3 and found, (rc, msg)
    need = int(found.group(1))
    print(f"{name}: needs {need} bytes, its size function returns {size}")
    assert 0 < need <= size and need % 256 == 0, (need, size)
    if name in ("rdrf_dynamic_bwd", "rdrf_dynamic_features_bwd"):      # the carves that decide the two maxima: one to one
        assert need == size, (need, size)
    assert untouched(), "the measuring call wrote a gradient"
    rc, msg, _ = backward(ws, need - 256)
    assert rc == -3 and "too small" in msg, (rc, msg)
    assert untouched(), "a refused backward wrote a gradient"
    assert bool((ws == CANARY).all()), "a refused backward wrote into the workspace"
    rc, msg, _ = backward(ws, need)
    assert rc == 0, (rc, msg)
    assert not untouched(), "the backward wrote no gradient"
    assert all(bool(torch.isfinite(t).all()) for t in gouts)
    assert bool((ws[need:] == CANARY).all()), f"{name}: written past the {need} bytes it asked for"
