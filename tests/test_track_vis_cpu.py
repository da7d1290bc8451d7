"""CPU-side checks of the per-slot visibility of point tracks (track_visibility / rdrf_track_visibility_fwd): the float64
reference of tests/_track_vis_prim.py against the oracle's compositor, the slot's ray and depth against the oracle's ray
generation and projection, the ABI additions, and the argument checks (which raise before any device work)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import _track_vis_prim as P
from _util import load_case, pkg
from oracle import rodynrf_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = {"ndc": "motion_ndc", "contract": "motion_contract"}
SHIFT = {"ndc": -2.0, "contract": -3.0}      # tests/test_gpu_track_vis.py SHIFT


def _oracle_ray_inputs(rt, S, n=48):
    """z, dists, sigma_s, sigma_d, blending [n,S] of the oracle's forward on rays of the motion fixture, float64"""
    g, sd_s, cfg_s, sd_d, cfg_d = load_case(CASE[rt])
    cfg_s, cfg_d = dict(cfg_s, density_shift=SHIFT[rt]), dict(cfg_d, density_shift=SHIFT[rt])
    rays, ts = torch.from_numpy(g["rays"])[::8][:n], torch.from_numpy(g["ts"])[::8][:n]
    nf = [float(v) for v in g["meta.near_far"]]
    xyz, z, valid = O.sampleXYZ(rays, cfg_d["aabb"], nf, S, rt)
    o_s = O.field_forward(sd_s, cfg_s, rays, ts, xyz, z, valid, rt, dynamic=False)
    o_d = O.field_forward(sd_d, cfg_d, rays, ts, xyz, z, valid, rt, dynamic=True)
    return tuple(t.double() for t in (z, o_d[9], o_s[7], o_d[7], o_d[2])), rays.double()


@pytest.mark.parametrize("rt", ["ndc", "contract"])
@pytest.mark.parametrize("S", [13, 65])
def test_reference_reproduces_t_full_at_every_sample(rt, S):
    (z, dists, ss, sd, b), rays = _oracle_ray_inputs(rt, S)
    n = z.shape[0]
    # T_full recovered in float64 from the oracle's own formula; and that formula IS what raw2outputs weighs with
    T = P.t_full(dists, ss, sd, b)
    outs = O.raw2outputs(torch.zeros(n, S, 3, dtype=torch.float64), ss, torch.zeros(n, S, 3, dtype=torch.float64), sd, dists, b, z,
                         rays, False, rt)
    a_d, a_s = 1.0 - torch.exp(-sd * dists), 1.0 - torch.exp(-ss * dists)
    assert float((outs[3] - (a_d * b + a_s * (1.0 - b)) * T).abs().max()) <= 1e-15
    for j in range(S):
        vis, jj = P.visibility(z, dists, ss, sd, b, z[:, j])
        assert bool((jj == j).all())
        # the partial factor at a sample position is F(0) = 1 + 1e-10
        assert float((vis - T[:, j] * (1.0 + 1e-10)).abs().max()) <= 4e-16, j
    assert float(T.min()) < 0.05 < 0.95 < float(T.max())


@pytest.mark.parametrize("rt", ["ndc", "contract"])
def test_reference_is_continuous_and_has_the_stated_ends(rt):
    S = 13
    (z, dists, ss, sd, b), _ = _oracle_ray_inputs(rt, S)
    n = z.shape[0]
    T = P.t_full(dists, ss, sd, b)
    for j in range(1, S):
        w = z[:, j] - z[:, j - 1]
        lo, jl = P.visibility(z, dists, ss, sd, b, z[:, j] - 1e-9 * w)
        hi, jh = P.visibility(z, dists, ss, sd, b, z[:, j] + 1e-9 * w)
        assert bool((jl == j - 1).all()) and bool((jh == j).all())
        assert float((lo - T[:, j]).abs().max()) <= 1e-7 and float((hi - T[:, j]).abs().max()) <= 1e-7, j
        mid, _ = P.visibility(z, dists, ss, sd, b, z[:, j - 1] + 0.5 * w)      # strictly between the ends where there is density
        assert bool((mid <= T[:, j - 1] * (1 + 1e-9)).all()) and bool((mid >= T[:, j] * (1 - 1e-9)).all())
    before, jb = P.visibility(z, dists, ss, sd, b, z[:, 0] - 0.25)
    assert bool((jb == -1).all()) and bool((before == 1.0).all())
    full = P.factor(ss, sd, b, dists).prod(-1)
    beyond, je = P.visibility(z, dists, ss, sd, b, z[:, -1] + 10.0)
    assert bool((je == S - 1).all()) and float((beyond - full).abs().max()) <= 1e-15


def test_inputs_exercise_the_product():
    """the density shifts of tests/test_gpu_track_vis.py: over depths spread along the rays the visibility covers (0, 1)"""
    for rt in ("ndc", "contract"):
        (z, dists, ss, sd, b), _ = _oracle_ray_inputs(rt, 64)
        T = P.t_full(dists, ss, sd, b)
        mid = float(((T > 0.05) & (T < 0.95)).double().mean())
        assert mid >= 0.2 and float(T.min()) < 0.01 and float(T.max()) > 0.99, (rt, mid, float(T.min()))


@pytest.mark.parametrize("rt", ["ndc", "contract"])
def test_the_point_lies_on_its_slot_ray_at_its_depth(rt):
    g = load_case(CASE[rt])[0]
    H, W, focal = int(g["meta.H"]), int(g["meta.W"]), float(g["focal"])
    c2w3 = torch.from_numpy(np.stack([g["c2w_b"], g["c2w"], g["c2w_f"]])).double()
    poses9 = P.poses9_of(c2w3)
    mtx = O.pose_to_mtx(poses9)
    gen = torch.Generator().manual_seed(7)
    n = 60
    view = torch.arange(n) % 3
    rays = torch.from_numpy(g["rays"]).double()[torch.randint(0, 384, (n,), generator=gen)]
    d = torch.rand(n, generator=gen).double()
    if rt == "ndc":
        p = rays[:, :3] + rays[:, 3:] * (0.02 + 0.96 * d)[:, None]
    else:
        p = O._linf_contract(rays[:, :3] + rays[:, 3:] * (0.1 + 6.0 * d)[:, None])
    pix, cam, zstar = P.slot_geometry(O, p, mtx[view], focal, H, W, rt)
    assert bool((cam[:, 2] < 0).all())
    # the pixel is render_single_3d_point's / render_3d_point's
    if rt == "ndc":
        want, disp = O.render_single_3d_point(H, W, focal, mtx[view], p)
    else:
        want, disp = O.render_3d_point(H, W, focal, mtx[view], torch.ones(n, 1, dtype=torch.float64), p[:, None], torch.zeros(n, 6, dtype=torch.float64),
                                       "contract")
    assert torch.equal(pix, want)
    slot_rays = O.generate_rays(view * (H * W), poses9, focal, H, W, ndc=rt == "ndc", near=1.0, uv=pix)
    on_ray = slot_rays[:, :3] + slot_rays[:, 3:] * zstar[:, None]
    if rt == "contract":
        on_ray = O._linf_contract(on_ray)
    scale = float(p.abs().max())
    assert float((on_ray - p).abs().max()) <= 1e-11 * scale, float((on_ray - p).abs().max())
    # the camera's own pixel centre gives the camera's own ray
    ids = torch.tensor([5 + 3 * W + H * W])
    own = O.generate_rays(ids, poses9, focal, H, W, ndc=rt == "ndc", near=1.0)
    same = O.generate_rays(ids, poses9, focal, H, W, ndc=rt == "ndc", near=1.0, uv=torch.tensor([[5.5, 3.5]], dtype=torch.float64))
    assert torch.equal(own, same)


def test_abi_additions():
    L = pkg()
    hdr = open(os.path.join(ROOT, "include", "rodynrf.h")).read()
    for sym in ("rdrf_track_visibility_ws_bytes", "rdrf_track_visibility_fwd"):
        assert re.search(r"\b" + sym + r"\s*\(", hdr), sym
        assert sym in L.SIGNATURES and hasattr(L.lib, sym), sym
    assert "#define RDRF_ABI_VERSION 6" in hdr and L.lib.rdrf_abi_version() == 6 == L.ABI_VERSION
    assert C.sizeof(L.TrackCamsC) == 32 and C.sizeof(L.TracksC) == 24           # the existing structs are untouched
    f = L.lib.rdrf_track_visibility_ws_bytes
    Ms, Ks, Ss = (0, 1, 31, 32, 33, 70, 4096, 65569), (1, 2, 9, 25, 100), (1, 13, 64, 65, 115, 440)
    size = {(m, k, s): int(f(m, k, s)) for m in Ms for k in Ks for s in Ss}
    assert all(v > 0 for v in size.values())
    for k in Ks:
        for s in Ss:
            col = [size[m, k, s] for m in Ms]
            assert col == sorted(col) and col[0] < col[-1]
    for m in Ms[1:]:
        for s in Ss:
            col = [size[m, k, s] for k in Ks]
            assert col == sorted(col) and col[0] < col[-1]
        for k in Ks:
            col = [size[m, k, s] for s in Ss]
            assert col == sorted(col) and col[0] < col[-1]


def test_package_surface():
    import rodynrf
    assert "track_visibility" in rodynrf.__all__ and hasattr(rodynrf, "track_visibility")
    sig = inspect.signature(rodynrf.track_visibility)
    assert list(sig.parameters) == ["tensorf_static", "tensorf", "tracks_or_points", "ts", "n_fwd", "n_bwd", "T", "cameras", "focal",
                                    "H", "W", "N_samples", "ray_type", "margin"]
    assert sig.parameters["N_samples"].default == -1 and sig.parameters["ray_type"].default == "ndc"
    assert sig.parameters["margin"].default == 0.0
    assert rodynrf.Tracks._fields == ("points", "pixels", "disp", "frames_offset")
    assert "no visibility along the track" not in rodynrf.track_points.__doc__ and "track_visibility" in rodynrf.track_points.__doc__


def test_argument_errors_come_before_device_work():
    """every tensor is on the CPU: a call that got as far as the device would raise RdrfError (no CPU fallback)"""
    import rodynrf
    pts, ts, cams = torch.zeros(4, 3, 3), torch.zeros(4), torch.eye(3, 4)[None].repeat(3, 1, 1)
    ok = dict(n_fwd=1, n_bwd=1, T=12, cameras=cams, focal=10.0, H=8, W=8)

    def call(points=pts, times=ts, **kw):
        a = dict(ok, **kw)
        return rodynrf.track_visibility(None, None, points, times, a["n_fwd"], a["n_bwd"], a["T"], a["cameras"], a["focal"], a["H"],
                                        a["W"], N_samples=13, ray_type=a.get("ray_type", "ndc"), margin=a.get("margin", 0.0))

    with pytest.raises(NotImplementedError):
        call(ray_type="world")
    for bad in (dict(n_fwd=-1), dict(n_bwd=-1), dict(n_fwd=2), dict(cameras=None), dict(cameras=cams[:2]), dict(cameras=torch.zeros(3, 4, 4)),
                dict(focal=None), dict(H=0), dict(W=None), dict(margin=float("nan")), dict(points=torch.zeros(4, 3)),
                dict(points=torch.zeros(4, 2, 3)), dict(times=torch.zeros(5)), dict(n_fwd=0, n_bwd=0, points=torch.zeros(4, 1, 3), T=1, cameras=cams[:2])):
        with pytest.raises(ValueError):
            call(**bad)
    with pytest.raises(ValueError):
        call(T=1)
    # the C entry point refuses what the track entry points refuse (no device is touched: the checks come first)
    L = pkg()
    PS, PD, cs, cd = L.RdrfStaticParams(), L.RdrfDynamicParams(), L.RdrfFieldCfg(), L.RdrfFieldCfg()
    cam = L.TrackCamsC(8, 8, 3, 1, 1)

    def c_call(M=0, n_fwd=1, n_bwd=1, S=13, cams_=cam, rt=(0, 0)):
        cs.ray_type, cd.ray_type = rt
        return L.lib.rdrf_track_visibility_fwd(C.byref(PS), C.byref(cs), C.byref(PD), C.byref(cd), None, None, M, n_fwd, n_bwd, 0.1,
                                               None if cams_ is None else C.byref(cams_), S, 0.0, 1.0, 0.0, None, None, 0, None)

    assert c_call() == 0                                            # M == 0: a no-op
    assert c_call(rt=(1, 1)) == 0
    for kw in (dict(rt=(2, 2)), dict(rt=(0, 1)), dict(n_fwd=-1), dict(S=0), dict(cams_=None), dict(n_fwd=2), dict(M=-1)):
        assert c_call(**kw) == -1, kw
        assert b"track_visibility" in L.lib.rdrf_last_error()
    assert c_call(M=3) == -1                                        # points, output and workspace are required once M > 0
