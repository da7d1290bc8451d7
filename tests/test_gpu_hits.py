"""Surface hits on the GPU (rdrf_hits_from_planes, rdrf_render_hits_fwd; render_hits, hit_view, render_hit_tracks,
point_cloud) against the float64 reference of tests/_hits_prim.py.

Residual bound of test 1.  With the kernel's own z_hit, the float64 visibility of the same planes (tests/_track_vis_prim.py)
differs from L by at most
        k 2^-24 max(L, m_j)  +  the reference's own change over z_hit -+ 1 ulp,
k counted from the kernel's operations in units of 2^-24, the largest relative error of one rounded fp32 operation:
  a factor F_s: _track_vis_prim's count for alpha_of and tfull_factor is 14 units ABSOLUTE (every quantity is <= 1); the kernel
    forms dists in fp32 -- three roundings and |d|'s three, 6 half-units on x = sigma d, at most x e^-x 3 <= 1.1 on each alpha,
    a convex combination on F: 2 more.  C_FACTOR = 16.  The compositor's 1 - alpha loses the RELATIVE precision of a small
    factor, so a factor's share of the product's relative error is C_FACTOR / F_s, and the product in front of the hit sample
    carries sum_{i < j} C_FACTOR / F_i.  These F_i exceed L / m_i, so the sum is bounded by the data, not by the result.
  the scan: a multiply per factor is in the 14; the carry into T once per round of 64: j // 64 + 1.
  the solver's last step: t is the smallest fp32 fraction at which the fp32 m_j F_j(t dists_j) <= L, so L lies between two
    fp32 evaluations one ulp of t apart: the true change over that ulp, x t e^-(x t) 2 units <= 1, and twice an evaluation
    (C_FACTOR, the rounding of t dists_j inside it, the product with m_j: 18); where t = 1 is taken because the scan said so,
    the scan's T_{j+1} and m_j F_j(dists_j) are two evaluations of the same number, the same 2 x 18.  The reference multiplies
    1 + 1e-10 per sample where fp32 rounds it away: S 1e-10 <= 1 unit.  C0 = 36 + 1 + 1 + 2 spare = 40.
  z_hit = z_j + t (z_{j+1} - z_j) is two rounded operations, at most one ulp of z_hit together; what that does to T depends on
    the slope, and is taken from the reference itself, as test_gpu_track_vis.py takes the rounding of its query depth.
Depth: |z_hit - z_ref| <= residual bound / slope + 2 ulp(z), on the rays above _hits_prim.SLOPE_FLOOR."""
import functools

import numpy as np
import pytest
import torch

import _hits_prim as H
import _track_vis_prim as P
import test_gpu_track_vis as V
import _util
from _twin import CHILD, assert_same_dict, run_twin, same_bits
from _util import RTOL, pkg, record_margin
from oracle import rodynrf_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"
U24 = H.U24
T8 = H.TAUS[8]


def same_hits(a, b):
    return all(same_bits(a[n], b[n]) for n in ("z", "hit", "xyz", "owner"))


def from_planes(rt, pl, tau, sel=None):
    rays, z, ss, sd, b = (t.to(DEV) if sel is None else t[sel].to(DEV) for t in pl)
    return _util.rodynrf().hits_from_planes(rays, z, ss, sd, b, tau=tau, ray_type=rt, distance_scale=H.DISTANCE_SCALE[rt])


check_against_reference = H.check_against_reference


# ---- 1. the kernel alone against the float64 reference -----------------------------------------------------------------
CASES1 = [(rt, S, N) for rt in ("ndc", "contract") for S in H.SHAPES_S for N in H.SHAPES_N]


@pytest.mark.parametrize("rt,S,N", CASES1, ids=[f"{a}-S{b}-N{c}" for a, b, c in CASES1])
def test_hits_from_planes_against_the_float64_reference(rt, S, N):
    pl = H.planes(rt, N, S)
    got = from_planes(rt, pl, T8)
    assert got["z"].shape == (8, N) and got["xyz"].shape == (8, N, 3) and got["hit"].dtype == torch.bool
    worst, n_hit, n_floor, n_clear, n_all = check_against_reference(rt, pl, got, T8, f"{rt} S={S} N={N}")
    print(f"{rt} S={S} N={N}: worst residual / bound {worst:.3f}; {n_hit} hits checked, {n_floor} under the slope floor, "
          f"{n_clear}/{n_all} clear of every crossing")
    if n_all >= 100:
        assert n_clear >= 0.9 * n_all
    if n_hit >= 50:
        assert n_floor <= H.FLOOR_CAP * n_hit
    # the levels of a call do not depend on each other (n_tau 1 and 3 are subsets of the 8), nor a ray on N or on the run
    for n_tau in (1, 3):
        sub = from_planes(rt, pl, H.TAUS[n_tau])
        rows = [T8.index(t) for t in H.TAUS[n_tau]]
        assert all(same_bits(sub[n], got[n][rows]) for n in ("z", "hit", "xyz", "owner")), n_tau
    one = from_planes(rt, pl, 0.5)
    assert one["z"].shape == (N,) and same_bits(one["z"], got["z"][3]) and same_bits(one["xyz"], got["xyz"][3])
    assert same_hits(from_planes(rt, pl, T8), got)
    for i in sorted({0, N // 2, N - 1}):
        alone = from_planes(rt, pl, T8, sel=slice(i, i + 1))
        assert all(same_bits(alone[n], got[n][:, i:i + 1]) for n in ("z", "hit", "xyz", "owner")), i
    # monotone in tau, bit for bit: the depth never falls, a ray that misses a level misses every later one
    zz, hh = got["z"], got["hit"]
    assert bool((zz[1:] >= zz[:-1]).all()) and bool((hh[1:].int() <= hh[:-1].int()).all())
    # the point is the sampler's arithmetic at z_hit (ndc: one multiply-add per component, no contraction)
    if rt == "ndc":
        rays = pl[0].to(DEV)
        want = rays[None, :, :3] + rays[None, :, 3:] * got["z"][..., None]
        assert same_bits(got["xyz"], want)


# ---- 2. regimes, each on the smallest shape that shows it --------------------------------------------------------------
def _ray(rt, S):
    rays = torch.tensor([[0.1, -0.2, -1.0 if rt == "ndc" else 0.3, 0.05, 0.02, 2.0 if rt == "ndc" else -1.0]])
    z = torch.linspace(0.0, 1.0, S)[None] if rt == "ndc" else (0.1 + torch.linspace(0.0, 1.5, S)[None])
    return rays, z.float().contiguous()


@pytest.mark.parametrize("rt", ["ndc", "contract"])
def test_regimes(rt):
    S = 13
    rays, z = _ray(rt, S)
    zero = torch.zeros(1, S)
    ds = float(H.dists_of(z, rays, H.DISTANCE_SCALE[rt])[0, 0])
    # empty space: every level misses
    got = from_planes(rt, (rays, z, zero, zero, zero), T8)
    assert not bool(got["hit"].any()) and bool((got["z"] == float(z[0, -1])).all()) and bool((got["owner"] == 0).all())
    # an opaque wall of the dynamic field in sample 4: every level lands in its first thousandth
    wall = zero.clone()
    wall[0, 4] = 1e5 / ds
    got = from_planes(rt, (rays, z, zero, wall, torch.ones(1, S)), T8)
    assert bool(got["hit"].all()) and bool((got["owner"] == 1).all())
    assert bool((got["z"] >= z[0, 4].item()).all()) and bool((got["z"] <= float(z[0, 4]) + 1e-3 * float(z[0, 5] - z[0, 4])).all())
    assert bool((got["z"][1:] >= got["z"][:-1]).all()) and float(got["z"][-1]) > float(got["z"][0])
    # an opaque FIRST sample: j = 0
    first = zero.clone()
    first[0, 0] = 1e5 / ds
    got = from_planes(rt, (rays, z, first, zero, zero), T8)
    assert bool(got["hit"].all()) and bool((got["owner"] == 0).all()) and bool((got["z"] <= float(z[0, 1])).all())
    # a floater (alpha 0.3, dynamic) in front of a wall (static): tau 0.1 lands on the floater, 0.9 on the wall
    sd, ss, b = zero.clone(), zero.clone(), zero.clone()
    sd[0, 3], b[0, 3] = -np.log(0.7) / ds, 1.0
    ss[0, 9] = 1e5 / ds
    got = from_planes(rt, (rays, z, ss, sd, b), (0.1, 0.9))
    assert bool(got["hit"].all())
    assert float(z[0, 3]) <= float(got["z"][0]) <= float(z[0, 4]) and float(got["owner"][0]) == 1.0
    assert float(z[0, 9]) <= float(got["z"][1]) <= float(z[0, 10]) and float(got["owner"][1]) == 0.0
    # a level only the last, zero-width sample could cross: its huge sigma meets dists = 0
    last = zero.clone()
    last[0, S - 1] = 1e5
    got = from_planes(rt, (rays, z, last, zero, zero), T8)
    assert not bool(got["hit"].any()) and bool((got["z"] == float(z[0, -1])).all())
    # NaN behind the crossing: no effect; before it: NaN and no hit
    sn = wall.clone()
    sn[0, 8] = float("nan")
    ref = from_planes(rt, (rays, z, zero, wall, torch.ones(1, S)), T8)
    assert same_hits(from_planes(rt, (rays, z, zero, sn, torch.ones(1, S)), T8), ref)
    half = zero.clone()
    half[0, 4] = -np.log(0.4) / ds                    # T falls to 0.4 in sample 4: tau up to 0.5 cross there, the others meet the NaN
    hn = half.clone()
    hn[0, 8] = float("nan")
    clean, got = from_planes(rt, (rays, z, zero, half, torch.ones(1, S)), T8), from_planes(rt, (rays, z, zero, hn, torch.ones(1, S)), T8)
    assert bool(clean["hit"][:4].all()) and not bool(clean["hit"][4:].any())
    assert all(same_bits(got[n][:4], clean[n][:4]) for n in ("z", "hit", "xyz", "owner"))
    assert not bool(got["hit"][4:].any()) and bool(torch.isnan(got["z"][4:]).all()) and bool(torch.isnan(got["xyz"][4:]).all())
    bn = torch.ones(1, S)
    bn[0, 2] = float("nan")                           # a NaN blending in front of everything
    got = from_planes(rt, (rays, z, zero, half, bn), T8)
    assert not bool(got["hit"].any()) and bool(torch.isnan(got["z"]).all())


@pytest.mark.parametrize("rt", ["ndc", "contract"])
def test_a_plateau_whose_scan_values_wobble_by_an_ulp_keeps_the_order(rt):
    """three samples with density, then 126 empty ones: the scan's T_s of the plateau differ in the last place from lane to lane
    (each lane's product associates differently), and levels placed a few ulps around the plateau either cross BEFORE it or
    miss; the running minimum keeps depth and flag in order"""
    S = 129
    rays, z = _ray(rt, S)
    ds = H.dists_of(z, rays, H.DISTANCE_SCALE[rt])[0]
    sd = torch.zeros(1, S)
    for s, a in ((0, 0.11), (1, 0.23), (2, 0.37)):
        sd[0, s] = float(-np.log(1.0 - a) / ds[s])
    plateau = float(np.float32((1 - 0.11) * (1 - 0.23) * (1 - 0.37)))
    grid = 2.0 ** -24                                  # the spacing of tau = 1 - L in [0.5, 1): both differences are exact there
    L0 = round(plateau / grid) * grid
    taus = sorted(1.0 - (L0 + k * grid) for k in (-32, -8, -2, -1, 1, 2, 8, 32))
    assert all(float(np.float32(t)) == t for t in taus)
    assert all(b > a for a, b in zip(taus, taus[1:]))
    got = from_planes(rt, (rays, z, torch.zeros(1, S), sd, torch.ones(1, S)), taus)
    zz, hh = got["z"][:, 0], got["hit"][:, 0]
    assert bool((zz[1:] >= zz[:-1]).all()) and bool((hh[1:].int() <= hh[:-1].int()).all())
    assert bool(hh[0]) and not bool(hh[-1])
    assert bool((zz[hh] <= float(z[0, 3])).all()) and bool((zz[~hh] == float(z[0, -1])).all())   # never ON the plateau


# ---- 3. the render entry point on the toy fields of the track-visibility tests -----------------------------------------
@functools.lru_cache(maxsize=None)
def batch(rt, n=96):
    g = V.scene(rt)[0]
    return torch.from_numpy(g["rays"])[:n].to(DEV).contiguous(), torch.from_numpy(g["ts"])[:n].to(DEV).contiguous()


@pytest.mark.parametrize("rt", ["ndc", "contract"])
@pytest.mark.parametrize("S", [13, 65])
def test_render_hits_paths_maps_and_planes(rt, S):
    rodynrf = _util.rodynrf()
    _, st, dy = V.scene(rt)[:3]
    rays, ts = batch(rt)
    dens = rodynrf.render_hits(st, dy, rays, ts, T8, N_samples=S, ray_type=rt)
    full = rodynrf.render_hits(st, dy, rays, ts, T8, N_samples=S, ray_type=rt, maps=True)
    assert same_hits(dens, full)                                     # the density-only path and the render give equal bits
    maps = rodynrf.render_rays(st, dy, rays, ts, N_samples=S, ray_type=rt, maps=True)
    for n in rodynrf.RenderMaps._fields:
        assert same_bits(full[n], getattr(maps, n)), n
    some = rodynrf.render_hits(st, dy, rays, ts, T8, N_samples=S, ray_type=rt, maps=("depth", "acc_d"))
    assert same_hits(some, full) and same_bits(some["depth"], maps.depth) and "rgb" not in some
    # the kernel alone on forward()'s own planes
    with torch.no_grad():
        xyz, z, valid = rodynrf.sampleXYZ(dy, rays, S, ray_type=rt, is_train=False)
        o_s = st(rays, ts, None, xyz, z, valid, ray_type=rt, N_samples=S, rgb=False)
        o_d = dy(rays, ts, None, xyz, z, valid, ray_type=rt, N_samples=S, rgb=False)
    alone = rodynrf.hits_from_planes(rays, z, o_s.sigma, o_d.sigma, o_d.blending, tau=T8, ray_type=rt, distance_scale=dy.distance_scale)
    assert same_hits(alone, dens)
    # a miss sits on the last sample, with that sample's bits
    miss = ~dens["hit"]
    assert bool(dens["hit"].any())
    assert same_bits(dens["xyz"][miss], xyz[:, -1][None].expand(8, -1, -1)[miss]) and bool((dens["z"][miss] == z[:, -1][None].expand(8, -1)[miss]).all())
    # against the float64 reference on these planes (the inputs of a trained-like field, not synthetic ones)
    pl = tuple(t.cpu() for t in (rays, z, o_s.sigma, o_d.sigma, o_d.blending))
    worst = check_against_reference(rt, pl, dens, T8, f"{rt} S={S} render_hits", scale=float(dy.distance_scale))[0]
    print(f"{rt} S={S}: render_hits worst residual / bound {worst:.3f}, hit share {float(dens['hit'].float().mean()):.2f}")


@pytest.mark.parametrize("rt", ["ndc", "contract"])
def test_hits_against_the_oracle_end_to_end(rt):
    """the oracle's own sigmas and blending through the float64 reference: the transmittance of the ORACLE's planes at the
    native z_hit equals L within RTOL, the bound test_visibility_against_the_oracle_end_to_end puts on its visibilities"""
    from _gpu_util import oracle_cfg, oracle_sd
    rodynrf = _util.rodynrf()
    g, st, dy = V.scene(rt)[:3]
    rays, ts = batch(rt, 24)
    S = 13
    taus = H.TAUS[3]
    got = rodynrf.render_hits(st, dy, rays, ts, taus, N_samples=S, ray_type=rt)
    r_, t_ = rays.cpu(), ts.cpu()
    nf = [float(v) for v in g["meta.near_far"]]
    xyz, z, valid = O.sampleXYZ(r_, dy.aabb.cpu(), nf, S, rt)
    o_s = O.field_forward(oracle_sd(st), oracle_cfg(st), r_, t_, xyz, z, valid, rt, dynamic=False)
    o_d = O.field_forward(oracle_sd(dy), oracle_cfg(dy), r_, t_, xyz, z, valid, rt, dynamic=True)
    worst = 0.0
    for k, tau in enumerate(taus):
        ref = H.hits(z, o_d[9], o_s[7], o_d[7], o_d[2], tau)
        hk = got["hit"][k].cpu()
        # flags agree wherever the oracle's transmittance stays RTOL away from L at every sample
        clear = ((ref["m"][:, 1:] - ref["L"]).abs() > RTOL).all(-1)
        assert bool((hk == ref["hit"])[clear].all())
        sel = clear & ref["hit"]
        vis, _ = P.visibility(z, o_d[9], o_s[7], o_d[7], o_d[2], torch.where(sel, got["z"][k].cpu().double(), z[:, 0].double()))
        if bool(sel.any()):
            worst = max(worst, float((vis - ref["L"]).abs()[sel].max()))
    print(f"{rt}: oracle transmittance at the native z_hit vs L: max err {worst:.3e}")
    record_margin(f"{rt} hits vs oracle end to end", worst / RTOL)
    assert worst <= RTOL


@pytest.mark.parametrize("rt", ["ndc", "contract"])
def test_batch_run_and_chunks_give_the_same_bits(rt, monkeypatch):
    rodynrf = _util.rodynrf()
    R = pkg("renderer")
    _, st, dy = V.scene(rt)[:3]
    rays, ts = batch(rt)
    S = 65
    whole = rodynrf.render_hits(st, dy, rays, ts, T8, N_samples=S, ray_type=rt, maps=("rgb",))
    assert same_hits(rodynrf.render_hits(st, dy, rays, ts, T8, N_samples=S, ray_type=rt, maps=("rgb",)), whole)
    for i in (0, 41, 95):
        alone = rodynrf.render_hits(st, dy, rays[i:i + 1], ts[i:i + 1], T8, N_samples=S, ray_type=rt)
        assert all(same_bits(alone[n], whole[n][:, i:i + 1]) for n in ("z", "hit", "xyz", "owner")), i
    one = rodynrf.render_hits(st, dy, rays, ts, 0.9, N_samples=S, ray_type=rt)
    assert all(same_bits(one[n], whole[n][5]) for n in ("z", "hit", "xyz", "owner"))
    monkeypatch.setattr(R, "_hits_chunk", lambda N, S: 37)
    parts = rodynrf.render_hits(st, dy, rays, ts, T8, N_samples=S, ray_type=rt, maps=("rgb",))
    assert same_hits(parts, whole) and same_bits(parts["rgb"], whole["rgb"])
    empty = rodynrf.render_hits(st, dy, rays[:0], ts[:0], T8, N_samples=S, ray_type=rt)
    assert empty["z"].shape == (8, 0) and empty["xyz"].shape == (8, 0, 3)


def det_case():
    """what both libraries compute (tests/_det_child.py case)"""
    rodynrf = _util.rodynrf()
    out = {}
    for rt in ("ndc", "contract"):
        _, st, dy = V.scene(rt)[:3]
        rays, ts = batch(rt)
        for S, maps in ((13, False), (65, ("rgb",))):
            h = rodynrf.render_hits(st, dy, rays, ts, T8, N_samples=S, ray_type=rt, maps=maps)
            for n in ("z", "hit", "xyz", "owner"):
                out[f"{rt}.{S}.{n}"] = h[n]
        pl = H.planes(rt, 257, 129)
        h = from_planes(rt, pl, T8)
        for n in ("z", "hit", "xyz", "owner"):
            out[f"{rt}.planes.{n}"] = h[n]
    return out


def test_deterministic_library_gives_the_same_bits(tmp_path):
    ours = det_case()
    assert_same_dict(run_twin(tmp_path, [CHILD, "case", "test_gpu_hits"], det=True), ours)


# ---- 4. what is built on the hits --------------------------------------------------------------------------------------
@pytest.mark.parametrize("rt", ["ndc", "contract"])
def test_hit_tracks_start_on_the_surface(rt):
    rodynrf = _util.rodynrf()
    st, dy, p9, focal, T, Hh, W, pixels = V.tiny_scene(rt)
    S, frame = 13, 2
    base = rodynrf.render_tracks(st, dy, p9, focal, frame, pixels, Hh, W, N_samples=S, ray_type=rt)
    hit = rodynrf.render_hit_tracks(st, dy, p9, focal, frame, pixels, Hh, W, N_samples=S, ray_type=rt, tau=0.3)
    again = rodynrf.render_tracks(st, dy, p9, focal, frame, pixels, Hh, W, N_samples=S, ray_type=rt)
    assert same_bits(again[0].points, base[0].points) and same_bits(again[1], base[1])       # render_tracks is what it was
    ids = pixels[:, 1] * W + pixels[:, 0] + frame * Hh * W
    rays = rodynrf.generate_rays(ids, p9, focal, Hh, W, ndc=rt == "ndc", near=1.0)
    ts = torch.full((pixels.shape[0],), 2.0 * frame / (T - 1) - 1.0, device=DEV)
    h = rodynrf.render_hits(st, dy, rays, ts, 0.3, N_samples=S, ray_type=rt)
    assert bool(h["hit"].any())
    want = torch.where(h["hit"][:, None], h["xyz"], base[0].points[:, frame])
    assert same_bits(hit[0].points[:, frame], want) and same_bits(hit[1], base[1])
    assert hit[0].points.shape == base[0].points.shape


@pytest.mark.parametrize("rt", ["ndc", "contract"])
def test_point_cloud_and_hit_view(rt):
    rodynrf = _util.rodynrf()
    st, dy, p9, focal, T, Hh, W, _ = V.tiny_scene(rt)
    c2w = rodynrf.pose_to_mtx(p9.detach().float())[2]
    S = 13
    hv = rodynrf.hit_view(st, dy, c2w, focal, Hh, W, 0.2, tau=0.3, N_samples=S, ray_type=rt, maps=("rgb", "depth"))
    assert hv["z"].shape == (Hh, W) and hv["xyz"].shape == (Hh, W, 3) and hv["rgb"].shape == (Hh, W, 3) and hv["hit"].dtype == torch.bool
    multi = rodynrf.hit_view(st, dy, c2w, focal, Hh, W, 0.2, tau=(0.3, 0.6), N_samples=S, ray_type=rt)
    assert multi["z"].shape == (2, Hh, W) and same_bits(multi["z"][0], hv["z"]) and same_bits(multi["xyz"][0], hv["xyz"])
    xyz, rgb, owner = rodynrf.point_cloud(st, dy, c2w, focal, Hh, W, 0.2, tau=0.3, N_samples=S, ray_type=rt)
    keep = hv["hit"].reshape(-1)
    assert 0 < int(keep.sum()) == xyz.shape[0]
    assert same_bits(xyz, hv["xyz"].reshape(-1, 3)[keep]) and same_bits(owner, hv["owner"].reshape(-1)[keep])
    assert same_bits(rgb, hv["rgb"].reshape(-1, 3)[keep].clamp(0.0, 1.0))
    dyn = rodynrf.point_cloud(st, dy, c2w, focal, Hh, W, 0.2, tau=0.3, N_samples=S, ray_type=rt, min_owner=0.5)
    sta = rodynrf.point_cloud(st, dy, c2w, focal, Hh, W, 0.2, tau=0.3, N_samples=S, ray_type=rt, max_owner=0.5)
    assert dyn[0].shape[0] + sta[0].shape[0] >= xyz.shape[0] and bool((dyn[2] >= 0.5).all()) and bool((sta[2] <= 0.5).all())
    # world space maps back into the field: the oracle's own inverse in float64 on the same fp32 points
    world = rodynrf.point_cloud(st, dy, c2w, focal, Hh, W, 0.2, tau=0.3, space="world", N_samples=S, ray_type=rt)[0].cpu().double()
    p64 = xyz.cpu().double()
    ref = O.ndc2world(p64, Hh, W, focal) if rt == "ndc" else O.contract2world(p64)
    # fp32 against float64: a handful of rounded operations, and the quotient 2 / (z - 1) (ndc) or 1 / (2 - n) (contract) carries
    # the relative error of its difference
    if rt == "ndc":
        cond = 1.0 + 1.0 / (p64[:, 2:].clamp(max=1 - 1e-6) - 1.0).abs()
    else:
        n = p64.abs().amax(-1, keepdim=True)
        cond = 1.0 + 1.0 / (2.0 - n.clamp(max=2.0 - 1e-6)).abs()
    assert bool(((world - ref).abs() <= 8 * U24 * cond * ref.abs().amax(-1, keepdim=True) + 1e-30).all())
