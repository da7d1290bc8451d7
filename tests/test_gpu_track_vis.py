"""Per-slot visibility of point tracks on the GPU (track_visibility / rdrf_track_visibility_fwd)
against the float64 reference of tests/_track_vis_prim.py.

Scene: the static + dynamic pair and the three cameras of tests/golden/motion_{ndc,contract}.npz, the cameras cycled over the
slots.  density_shift is lowered (SHIFT) until a ray's optical depth is of order 5: random-initialised fields at the
fixtures' own shift are opaque after two samples (checked with the oracle on the CPU: T_full spans 1 .. 1e-3 over the depths
used here, test_track_vis_cpu.py::test_inputs_exercise_the_product).  The seeds lie on the centre camera's rays at depths spread
over the sampled range; the first ones at its very start.

Bound of test 1, |vis - ref| <= (C_FACTOR (j + 1) + C0 + j // 64) 2^-24 + the first-order term of zq's rounding.
The reference is fed the z_vals, dists, sigma and blending of the project's own forward(rgb=False) on host-built rays, so what
is left is the kernel's arithmetic on top of them.  Every quantity below is <= 1 (+1e-10), so relative roundings are absolute;
the unit is 2^-24, the largest relative error of one rounded fp32 operation.
  per factor F_s: sigma * d: 1 rounding, an error x e^-x <= 0.37 of it in e^-x; expf: 2 ulp = 4 units (the constant of
    tests/_comp_prim.py); 1 - e: 1.  alpha carries <= 6 units, for either field.  dF = -b v dalpha_d - (1 - b) u dalpha_s with
    u, v <= 1: a convex combination, <= 6.  Then alpha_d * b, 1 - ., 1 - b, alpha_s * (1 - b), 1 - ., u * v, + 1e-10: 7, and the
    factor's multiply into the scan: 1 (a product of n factors takes n - 1 multiplies however the scan associates it).
    C_FACTOR = 14.
  the partial factor F_j counts as one more factor (the j + 1), and its d = fl(fl(fl(zq - z_j) |d|) scale) carries 3 roundings
    against the reference's fraction of forward()'s dists_j, which itself carries 3 and |d|'s 2: 8 units on x, 0.37 * 8 = 3 on
    each alpha, <= 3 on the factor.  The multiply of the round's carry into T: 1 per round of 64 (the j // 64 + 1), T * F_j: 1.
    C0 = 3 + 1 + 1 = 5.
  zq: the kernel forms it in fp32, the reference in float64 from the same points.  Its rounding bound dz is
    _track_vis_prim.zq_rounding; the term is max |ref(zq +- dz) - ref(zq)|, the reference's own change over that interval."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import _track_vis_prim as P
import _util
from _twin import CHILD, assert_same_dict, run_twin, same_bits
from _util import GOLDEN, RTOL, load_case, pkg, record_margin
from oracle import rodynrf_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"
T_VIDEO = 12
STEPS = ((0, 0), (1, 0), (0, 1), (5, 3))
SIZES = (1, 31, 32, 33, 70)
SAMPLES = (13, 64, 65)
SHIFT = {"ndc": -2.0, "contract": -3.0}
CASE = {"ndc": "motion_ndc", "contract": "motion_contract"}
C_FACTOR, C0 = 14, 5
U24 = 2.0 ** -24


def scan_geometry():
    """(slots per workgroup pass, workgroup cap) of k_track_vis_scan, read from the source"""
    src = open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "robust-dynrf_amd", "csrc", "rdrf_track_vis.hip")).read()
    return (int(re.search(r"constexpr int VIS_SCAN_WAVES = (\d+);", src).group(1)),
            int(re.search(r"constexpr int VIS_SCAN_MAX_BLOCKS = (\d+);", src).group(1)))


def _m_multi(K=9):
    """the smallest M (at K slots) at which a wave of k_track_vis_scan takes a second slot"""
    waves, blocks = scan_geometry()
    return (waves * blocks) // K + 1


M_MULTI = _m_multi()


@functools.lru_cache(maxsize=None)
def scene(rt, shift=None, blend_bias=None):
    """blend_bias: the blending head puts out this constant before its sigmoid (40: blending is exactly 1).
    (g, static field, dynamic field, cams [9,3,4] on the device, poses9 [3,9] + slot -> camera table on the host, focal, H, W)"""
    from _gpu_util import COMMON
    rodynrf = _util.rodynrf()
    g, sd_s, _, sd_d, _ = load_case(CASE[rt])
    kw = dict(COMMON, near_far=[float(v) for v in g["meta.near_far"]], density_shift=SHIFT[rt] if shift is None else shift,
              fea2denseAct=str(g["meta.act"]))
    aabb, grid = torch.from_numpy(g["aabb"]), [int(v) for v in g["meta.grid"]]
    st = rodynrf.TensorVMSplit(aabb, grid, 12, DEV, shadingMode=str(g["meta.static_head"]), fea_pe=2, **kw)
    dy = rodynrf.TensorVMSplit_TimeEmbedding(aabb, grid, 12, DEV, shadingMode="MLP_Fea_late_view", fea_pe=0, **kw)
    st.load_state_dict(sd_s)
    dy.load_state_dict(sd_d)
    if blend_bias is not None:
        with torch.no_grad():
            dy.blending_layer2.weight.zero_()
            dy.blending_layer2.bias.fill_(blend_bias)
    poses9 = P.poses9_of(torch.from_numpy(np.stack([g["c2w_b"], g["c2w"], g["c2w_f"]])))
    table = torch.tensor([0, 1, 2, 1, 0, 1, 2, 1, 0])
    cams = O.pose_to_mtx(poses9)[table]      # the matrices oracle.generate_rays builds from these poses, bit for bit
    return g, st, dy, cams.to(DEV), (poses9, table), float(g["focal"]), int(g["meta.H"]), int(g["meta.W"])


@functools.lru_cache(maxsize=None)
def seeds(rt, M):
    """M seed points on the centre camera's rays, depths spread over the sampled range (the first four at its start), and their
    times"""
    g = scene(rt)[0]
    gen = torch.Generator().manual_seed(4242 + M + (0 if rt == "ndc" else 1))
    rays = torch.from_numpy(g["rays"])
    rays = rays[torch.randint(0, rays.shape[0], (M,), generator=gen)]
    d = torch.rand(M, generator=gen)
    if rt == "ndc":
        d[:4] = 0.0
        p = rays[:, :3] + rays[:, 3:] * d[:, None]
    else:
        d = 0.05 + 7.0 * d ** 2
        d[:4] = 0.01
        p = O._linf_contract(rays[:, :3] + rays[:, 3:] * d[:, None])
    t = torch.randint(3, 7, (M,), generator=gen).float() * 2 / (T_VIDEO - 1) - 1
    return p.to(DEV), t.to(DEV)


def step_of(rt, S):
    """one sample step in z_vals units (contract: of the inner half, [near, 2] in S - S // 2 steps)"""
    return 1.0 / (S - 1) if rt == "ndc" else 2.0 / (S - S // 2)


def tracks_of(rt, M, n_fwd, n_bwd):
    rodynrf = _util.rodynrf()
    _, st, dy, cams, _, focal, H, W = scene(rt)
    p0, t0 = seeds(rt, M)
    K = n_bwd + 1 + n_fwd
    tr = rodynrf.track_points(dy, p0, t0, n_fwd, n_bwd, T_VIDEO, cameras=cams[:K], focal=focal, H=H, W=W, ray_type=rt)
    return tr, t0, cams[:K]


def native(rt, tr, t0, cams, n_fwd, n_bwd, S, margin, fields=None):
    rodynrf = _util.rodynrf()
    _, st, dy, _, _, focal, H, W = scene(rt)
    if fields is not None:
        st, dy = fields
    return rodynrf.track_visibility(st, dy, tr, t0, n_fwd, n_bwd, T_VIDEO, cams, focal, H, W, N_samples=S, ray_type=rt,
                                    margin=margin)


def slot_times(t0, n_fwd, n_bwd):
    """the chain's times in fp32, one rounded sum per step"""
    dt = torch.tensor(2.0 / (T_VIDEO - 1), dtype=torch.float32)
    K = n_bwd + 1 + n_fwd
    ts = [None] * K
    ts[n_bwd] = t0.clone()
    for k in range(1, n_fwd + 1):
        ts[n_bwd + k] = ts[n_bwd + k - 1] + dt
    for k in range(1, n_bwd + 1):
        ts[n_bwd - k] = ts[n_bwd - k + 1] - dt
    return torch.stack(ts, 1)


def reference(rt, tr, t0, n_fwd, n_bwd, S, margin, fields=None):
    """float64 reference on the project's own forward(rgb=False) outputs for host-built rays -> dict of [M*K] arrays"""
    rodynrf = _util.rodynrf()
    _, st, dy, cams, (poses9, table), focal, H, W = scene(rt)
    if fields is not None:
        st, dy = fields
    K = n_bwd + 1 + n_fwd
    M = tr.points.shape[0]
    pix = tr.pixels.cpu().reshape(M * K, 2)
    view = table[:K][None].expand(M, K).reshape(-1)
    rays = O.generate_rays(view * (H * W), poses9, focal, H, W, ndc=rt == "ndc", near=1.0, uv=pix)
    ts = slot_times(t0.cpu(), n_fwd, n_bwd).reshape(-1)
    with torch.no_grad():
        r, t = rays.to(DEV), ts.to(DEV)
        xyz, z, valid = rodynrf.sampleXYZ(dy, r, S, ray_type=rt, is_train=False)
        o_s = st(r, t, None, xyz, z, valid, ray_type=rt, N_samples=S, rgb=False)
        o_d = dy(r, t, None, xyz, z, valid, ray_type=rt, N_samples=S, rgb=False)
    p64 = tr.points.cpu().double().reshape(M * K, 3)
    c64 = cams[:K].cpu().double()[None].expand(M, K, 3, 4).reshape(M * K, 3, 4)
    _, cam, zstar = P.slot_geometry(O, p64, c64, focal, H, W, rt)
    zq = zstar - float(np.float32(margin))
    world = O.ndc2world(p64, H, W, focal) if rt == "ndc" else O.contract2world(p64)
    cam_terms = ((world.abs() + c64[..., 3].abs()) * c64[..., :3, 2].abs()).sum(-1)
    dz = P.zq_rounding(cam_terms, zstar, zq, rt)
    args = (z.cpu(), o_d.dists.cpu(), o_s.sigma.cpu(), o_d.sigma.cpu(), o_d.blending.cpu())
    ref, j = P.visibility(*args, zq)
    lo, _ = P.visibility(*args, zq - dz)
    hi, _ = P.visibility(*args, zq + dz)
    behind = cam[:, 2] >= 0
    ref = torch.where(behind, torch.zeros_like(ref), ref)
    return dict(ref=ref, j=j, zterm=torch.maximum((lo - ref).abs(), (hi - ref).abs()), behind=behind, zq=zq, z=z.cpu().double(),
                valid=valid.cpu())


# ---- 1. against the float64 reference ----------------------------------------------------------------------------------
CASES1 = [(rt, M, nf, nb, S) for rt in ("ndc", "contract") for M, (nf, nb), S in
          [(1, (0, 0), 13), (31, (1, 0), 64), (32, (0, 1), 65), (33, (5, 3), 13), (70, (5, 3), 64), (70, (5, 3), 65),
           (70, (0, 0), 13), (31, (5, 3), 65), (32, (1, 0), 13), (33, (0, 1), 64), (1, (5, 3), 65)]]
CASES1 += [(rt, M_MULTI, 5, 3, 13) for rt in ("ndc", "contract")]


@pytest.mark.parametrize("rt,M,n_fwd,n_bwd,S", CASES1, ids=[f"{a}-{b}-{c}f{d}b-S{e}" for a, b, c, d, e in CASES1])
def test_visibility_against_the_float64_reference(rt, M, n_fwd, n_bwd, S):
    waves, blocks = scan_geometry()
    K = n_bwd + 1 + n_fwd
    assert (M * K > waves * blocks) == (M == M_MULTI), "M_MULTI no longer is the case in which a wave takes a second slot"
    tr, t0, cams = tracks_of(rt, M, n_fwd, n_bwd)
    for margin in (0.0, 2.0 * step_of(rt, S)):
        got = native(rt, tr, t0, cams, n_fwd, n_bwd, S, margin)
        assert got.shape == (M, K) and bool(torch.isfinite(got).all())
        r = reference(rt, tr, t0, n_fwd, n_bwd, S, margin)
        jj = r["j"].clamp(min=0).double()
        bound = (C_FACTOR * (jj + 1) + C0 + torch.div(jj, 64, rounding_mode="floor")) * U24 + r["zterm"]
        err = (got.cpu().double().reshape(-1) - r["ref"]).abs()
        worst = int(torch.argmax(err / bound))
        print(f"{rt} M={M} K={K} S={S} margin={margin:.4f}: max err {float(err.max()):.3e}, worst err/bound "
              f"{float(err[worst] / bound[worst]):.3f} at j={int(r['j'][worst])} (zq term {float(r['zterm'][worst]):.2e})")
        record_margin(f"{rt} M={M} K={K} S={S} margin={margin:.4f} vis vs float64 reference", float((err / bound).max()))
        assert bool((err <= bound).all()), (rt, M, S, margin, float(err[worst]), float(bound[worst]))
        if M == 70 and (n_fwd, n_bwd) == (5, 3) and margin == 0.0:   # the inputs exercise the product
            v = r["ref"][~r["behind"]]
            mid = float(((v > 0.05) & (v < 0.95)).double().mean())
            print(f"{rt} S={S}: reference in (0.05, 0.95): {mid:.2f}, min {float(v.min()):.2e}, max {float(v.max()):.6f}")
            assert mid >= 0.2 and bool((v < 0.01).any()) and bool((v > 0.99).any())


# ---- 2. against the oracle end to end ----------------------------------------------------------------------------------
@pytest.mark.parametrize("rt", ["ndc", "contract"])
def test_visibility_against_the_oracle_end_to_end(rt):
    from _gpu_util import oracle_cfg, oracle_sd
    g, st, dy, cams, (poses9, table), focal, H, W = scene(rt)
    M, n_fwd, n_bwd, S = 8, 1, 1, 13
    K = 3
    tr, t0, cm = tracks_of(rt, M, n_fwd, n_bwd)
    margin = 2.0 * step_of(rt, S)
    got = native(rt, tr, t0, cm, n_fwd, n_bwd, S, margin).cpu().double().reshape(-1)
    pix = tr.pixels.cpu().reshape(M * K, 2)
    view = table[:K][None].expand(M, K).reshape(-1)
    rays = O.generate_rays(view * (H * W), poses9, focal, H, W, ndc=rt == "ndc", near=1.0, uv=pix)
    ts = slot_times(t0.cpu(), n_fwd, n_bwd).reshape(-1)
    nf = [float(v) for v in g["meta.near_far"]]
    xyz, z, valid = O.sampleXYZ(rays, dy.aabb.cpu(), nf, S, rt)
    o_s = O.field_forward(oracle_sd(st), oracle_cfg(st), rays, ts, xyz, z, valid, rt, dynamic=False)
    o_d = O.field_forward(oracle_sd(dy), oracle_cfg(dy), rays, ts, xyz, z, valid, rt, dynamic=True)
    p64 = tr.points.cpu().double().reshape(M * K, 3)
    c64 = cm.cpu().double()[None].expand(M, K, 3, 4).reshape(M * K, 3, 4)
    _, cam, zstar = P.slot_geometry(O, p64, c64, focal, H, W, rt)
    ref, _ = P.visibility(z, o_d[9], o_s[7], o_d[7], o_d[2], zstar - float(np.float32(margin)))
    ref = torch.where(cam[:, 2] >= 0, torch.zeros_like(ref), ref)
    err = float((got - ref).abs().max())
    print(f"{rt}: native vs oracle pipeline max err {err:.3e} (vis in [{float(ref.min()):.3f}, {float(ref.max()):.3f}])")
    record_margin(f"{rt} vis vs oracle end to end", err / RTOL)
    assert err <= RTOL


# ---- 3. bit identities -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rt", ["ndc", "contract"])
def test_a_slot_does_not_depend_on_its_batch_or_on_the_run(rt):
    S, margin = 64, 2.0 * step_of(rt, 64)
    tr, t0, cams = tracks_of(rt, 70, 5, 3)
    whole = native(rt, tr, t0, cams, 5, 3, S, margin)
    assert same_bits(native(rt, tr, t0, cams, 5, 3, S, margin), whole)
    for i in (0, 17, 69):
        alone = native(rt, tr.points[i:i + 1], t0[i:i + 1], cams, 5, 3, S, margin)
        assert same_bits(alone, whole[i:i + 1]), i
    for k in (0, 3, 8):   # one slot of one point: its own camera and its own time
        t_k = slot_times(t0.cpu(), 5, 3)[:, k].to(DEV)
        alone = native(rt, tr.points[5:6, k:k + 1], t_k[5:6], cams[k:k + 1], 0, 0, S, margin)
        assert same_bits(alone, whole[5:6, k:k + 1]), k


@pytest.mark.parametrize("rt", ["ndc", "contract"])
def test_chunked_calls_give_the_same_bits(rt, monkeypatch):
    R = pkg("renderer")
    S, margin = 13, 0.0
    tr, t0, cams = tracks_of(rt, 70, 5, 3)
    whole = native(rt, tr, t0, cams, 5, 3, S, margin)
    monkeypatch.setattr(R, "_track_vis_chunk", lambda M, K, S, H, W: 32)
    assert same_bits(native(rt, tr, t0, cams, 5, 3, S, margin), whole)


def det_case():
    """what both libraries compute (tests/_det_child.py case)"""
    out = {}
    for rt in ("ndc", "contract"):
        tr, t0, cams = tracks_of(rt, 70, 5, 3)
        for S in (13, 65):
            out[f"{rt}.{S}"] = native(rt, tr, t0, cams, 5, 3, S, 2.0 * step_of(rt, S))
    return out


def test_deterministic_library_gives_the_same_bits(tmp_path):
    ours = det_case()
    assert_same_dict(run_twin(tmp_path, [CHILD, "case", "test_gpu_track_vis"], det=True), ours)


@functools.lru_cache(maxsize=None)
def tiny_scene(rt):
    from _gpu_util import COMMON
    rodynrf = _util.rodynrf()
    torch.manual_seed(31)
    aabb = torch.tensor([[-1.5, -1.67, -1.0], [1.5, 1.67, 1.0]]) if rt == "ndc" else torch.tensor([[-2.0] * 3, [2.0] * 3])
    kw = dict(COMMON, near_far=[0.0, 1.0] if rt == "ndc" else [0.0, 256.0], density_shift=-2.0, fea2denseAct="softplus")
    grid = [17, 19, 11]
    st = rodynrf.TensorVMSplit(aabb, grid, 12, DEV, shadingMode="MLP_Fea", fea_pe=2, **kw)
    dy = rodynrf.TensorVMSplit_TimeEmbedding(aabb, grid, 12, DEV, shadingMode="MLP_Fea_late_view", fea_pe=0, **kw)
    T, H, W = 6, 12, 16
    g = torch.Generator().manual_seed(32)
    p9 = torch.zeros(T, 9)
    p9[:, 0] = 1
    p9[:, 4] = 1
    p9 = (p9 + 0.03 * torch.randn(T, 9, generator=g)).to(DEV)
    focal = max(H, W) / 2.0 * 1.7320508
    flat = torch.randperm(H * W, generator=g)[:40]
    pixels = torch.stack([flat % W, flat // W], -1).to(DEV)
    return st, dy, p9, focal, T, H, W, pixels


@pytest.mark.parametrize("rt", ["ndc", "contract"])
def test_visibility_of_render_tracks_own_tracks(rt):
    """render_tracks' Tracks go into track_visibility as they are, with the cameras and times its docstring names"""
    rodynrf = _util.rodynrf()
    st, dy, p9, focal, T, H, W, pixels = tiny_scene(rt)
    S, frame = 13, 2
    margin = 3.0 * step_of(rt, S)
    tracks, acc_d = rodynrf.render_tracks(st, dy, p9, focal, frame, pixels, H, W, N_samples=S, ray_type=rt)
    n_bwd, n_fwd = -int(tracks.frames_offset[0]), int(tracks.frames_offset[-1])
    assert (n_bwd, n_fwd) == (frame, T - 1 - frame)
    ts = torch.full((40,), 2.0 * frame / (T - 1) - 1.0, device=DEV)
    cams = rodynrf.pose_to_mtx(p9.detach().float())[frame - n_bwd: frame + n_fwd + 1]
    vis = rodynrf.track_visibility(st, dy, tracks, ts, n_fwd, n_bwd, T, cams, focal, H, W, N_samples=S, ray_type=rt, margin=margin)
    assert vis.shape == (40, T) and bool(torch.isfinite(vis).all()) and bool(((vis >= 0) & (vis <= 1)).all())
    assert same_bits(vis, rodynrf.track_visibility(st, dy, tracks.points, ts, n_fwd, n_bwd, T, cams, focal, H, W, N_samples=S,
                                               ray_type=rt, margin=margin))
    again = rodynrf.render_tracks(st, dy, p9, focal, frame, pixels, H, W, N_samples=S, ray_type=rt)   # the render is left as it was
    assert same_bits(again[0].points, tracks.points) and same_bits(again[1], acc_d)
    # a seed sits inside the density that defines it: with the margin it is seen better than without
    raw = rodynrf.track_visibility(st, dy, tracks, ts, n_fwd, n_bwd, T, cams, focal, H, W, N_samples=S, ray_type=rt)
    assert bool((raw <= vis).all()) and float(raw[:, frame].mean()) < float(vis[:, frame].mean())


# ---- 4. regimes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rt", ["ndc", "contract"])
def test_regimes(rt):
    rodynrf = _util.rodynrf()
    S = 13
    tr, t0, cams = tracks_of(rt, 70, 5, 3)
    _, st, dy, _, _, focal, H, W = scene(rt)
    # empty space: softplus(f - 60) underflows to exactly 0 in both fields
    empty = scene(rt, -60.0)[1:3]
    vis = native(rt, tr, t0, cams, 5, 3, S, 0.0, fields=empty)
    r = reference(rt, tr, t0, 5, 3, S, 0.0, fields=empty)
    front = ~r["behind"].reshape(70, 9).to(DEV)
    assert bool(front.any()) and bool((vis[front] == 1.0).all())
    # a wall: every sample opaque.  Where both fields are opaque the compositor's factor is b (1 - b) + 1e-10, which is 0.25 at
    # b = 0.5 and not 0 (renderer.py:236-245 lets light through two blended walls), so the wall is the dynamic field's: b = 1
    wall = scene(rt, 12.0, 40.0)[1:3]
    vis = native(rt, tr, t0, cams, 5, 3, S, 0.0, fields=wall).cpu().reshape(-1)
    r = reference(rt, tr, t0, 5, 3, S, 0.0, fields=wall)
    nvalid_before = ((r["z"] < r["zq"][:, None]) & r["valid"]).sum(-1)
    past = (nvalid_before >= 2) & ~r["behind"]                # zq lies past the second valid sample: one whole opaque interval
    assert int(past.sum()) > 100
    assert bool((vis[past] < 1e-6).all()), float(vis[past].max())
    # zq <= z_0: exactly 1 (the first four seeds sit at the start of the sampled range; a margin moves every point in front of it)
    vis = native(rt, tr, t0, cams, 5, 3, S, 0.0)
    r = reference(rt, tr, t0, 5, 3, S, 0.0)
    at0 = ((r["j"] <= 0) & ((r["zq"] <= r["z"][:, 0]) | (r["j"] < 0)) & ~r["behind"]).reshape(70, 9)
    assert int(at0.sum()) >= 4 and bool((vis.cpu()[at0] == 1.0).all())
    big = native(rt, tr, t0, cams, 5, 3, S, 1e4)
    assert bool((big[front] == 1.0).all())
    # a camera turned away from the point: exactly 0
    away = cams.clone()
    away[:, :, :3] = -away[:, :, :3]                          # looks the other way from the same place (cam = -cam)
    back = native(rt, tr, t0, away, 5, 3, S, 0.0)
    assert bool((back[front] == 0.0).all())
    # non-increasing as the margin decreases
    steps = [step_of(rt, S) * m for m in (6.0, 4.0, 3.0, 2.0, 1.0, 0.5, 0.0, -1.0)]
    seq = [native(rt, tr, t0, cams, 5, 3, S, m) for m in steps]
    for a, b in zip(seq, seq[1:]):
        assert bool((b <= a).all())
    assert bool((seq[-1] < seq[0]).any())
    # M = 0
    e = rodynrf.track_visibility(st, dy, tr.points[:0], t0[:0], 5, 3, T_VIDEO, cams, focal, H, W, N_samples=S, ray_type=rt)
    assert e.shape == (0, 9) and e.dtype == torch.float32
