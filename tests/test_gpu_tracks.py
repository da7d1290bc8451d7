"""Point tracks on the GPU (track_points / rdrf_track_points_fwd, render_tracks, get_forward_backward_scene_flow_point_single)
against the composition of public calls that defines them -- get_forward_backward_scene_flow on [M,1,3], add, clamp,
render_single_3d_point / render_3d_point -- bit for bit, and against the reference-generated fixture tests/golden/tracks.npz
(tests/golden/make_golden_tracks.py).

Bound of a chain against the fixture (test 3).  One step is p + sf(p, t): the project's forward tolerance for one evaluation of
an MLP against the reference is 1e-4 of the tensor's max (tests/_util.RTOL, the bound tests/test_gpu_flow.py and
tests/test_gpu_forward.py hold the single step to), and the step map is 1-Lipschitz to first order (|d sf / d p| << 1 in the
fixture: a step moves a point by ~0.05 over a box of size 3), so after k steps the error is at most k single-step errors:
    |pts_k - ref_k| <= k * 1e-4 * max|ref pts|,   slot of the seed: exact,
and the projection of slot k adds one more evaluation: (k + 1) * 1e-4 * max|ref| for pix and disp.  That is the bound of the
COMPOSITION of public calls.  The native chain is not given this room: per output and slot its error against the fixture
must not exceed the error the composition shows there in the same run -- the composition's measured margin plus nothing."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import _util
from _twin import CHILD, assert_same_dict, run_twin
from _util import GOLDEN, assert_close, pkg, record_margin

pytestmark = pytest.mark.gpu

DEV = "cuda"
RTOL = 1e-4            # the forward tolerance of the golden comparisons in tests/test_gpu_flow.py
LO, HI = -2.0 + 1e-6, 2.0 - 1e-6
T_VIDEO = 12
STEPS = ((0, 0), (1, 0), (0, 1), (5, 3))


def launch_geometry(M):
    """(workgroups, waves per workgroup, 32-point tiles) of k_track_points for M points: geo_for_units of csrc/rdrf_host.hpp,
    with its two constants read from the sources (RDRF_MAXW: csrc/rdrf_common.hpp; the workgroup cap `ncu`: geo_for_units)"""
    csrc = os.path.join(os.path.dirname(GOLDEN), os.pardir, "robust-dynrf_amd", "csrc")
    maxw = int(re.search(r"#define RDRF_MAXW (\d+)", open(os.path.join(csrc, "rdrf_common.hpp")).read()).group(1))
    body = re.search(r"Geo geo_for_units\(long units\) \{(.*?)\n\}", open(os.path.join(csrc, "rdrf_host.hpp")).read(), re.S).group(1)
    ncu = int(re.search(r"const int ncu = (\d+);", body).group(1))
    tiles = (M + 31) // 32
    waves = min(max((tiles + ncu - 1) // ncu, 1), maxw)
    grid = min(max((tiles + waves - 1) // waves, 1), ncu)
    return grid, waves, tiles


def _m_multi():
    """the smallest M at which some wave takes a second tile, plus a full tile and one point: a partial last tile on a second pass"""
    grid, waves, _ = launch_geometry(1 << 30)     # the caps
    return 32 * grid * waves + 33


M_MULTI = _m_multi()
SIZES = (1, 31, 32, 33, 70)


@functools.lru_cache(maxsize=None)
def fixture():
    z = np.load(os.path.join(GOLDEN, "tracks.npz"))
    return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def field(rt):
    from _gpu_util import COMMON
    rodynrf = _util.rodynrf()
    z = fixture()
    kw = dict(COMMON, near_far=[0.0, 1.0] if rt == "ndc" else [0.0, 256.0], density_shift=float(z["meta.density_shift"]),
              fea2denseAct=str(z["meta.act"]))
    dy = rodynrf.TensorVMSplit_TimeEmbedding(torch.from_numpy(z[rt + ".aabb"]), [int(v) for v in z["meta.grid"]], 12, DEV,
                                             shadingMode="MLP_Fea_late_view", fea_pe=0, **kw)
    dy.load_state_dict({k[2:]: torch.from_numpy(np.array(v)) for k, v in z.items() if k.startswith("d.")})
    return dy


def cameras():
    z = fixture()
    return torch.from_numpy(z["cams"]).to(DEV), float(z["focal"]), int(z["meta.H"]), int(z["meta.W"])


@functools.lru_cache(maxsize=None)
def seeds(rt, M):
    """M seeded points in the field's box and their times (frames 3 .. 6 of 12); from 31 points on the last rows hold the edge
    cases -- ndc: z at / next to 1 (NDC2world clamps z to 1 - 1e-6), contract: components at +-1.99 (the step clamp fires)"""
    g = torch.Generator().manual_seed(977 + M + (0 if rt == "ndc" else 1))
    lo, hi = torch.from_numpy(fixture()[rt + ".aabb"])
    p = lo + (hi - lo) * torch.rand(M, 3, generator=g)
    if rt == "contract":
        p = 0.95 * p
    if M >= 31:
        if rt == "ndc":
            p[-8:, 2] = torch.tensor([1.0, 0.9999999, 0.999999, 0.99999, 1.0 + 1e-6, 0.9999995, 0.999, 1.01])
        else:
            p[-6:] = 1.99 * torch.sign(p[-6:])
            p[-10:-6, 0] = -1.99
    t = torch.randint(3, 7, (M,), generator=g).float() * 2 / (T_VIDEO - 1) - 1
    return p.to(DEV), t.to(DEV)


def compose(dy, p0, t0, n_fwd, n_bwd, rt, cams=None, focal=None, H=None, W=None):
    """the chain by public calls, one launch sequence per step and slot"""
    rodynrf = _util.rodynrf()
    M, K = p0.shape[0], n_bwd + 1 + n_fwd
    dt = 2.0 / (T_VIDEO - 1)
    pts = [None] * K
    pts[n_bwd] = p0
    with torch.no_grad():
        for d, n in ((0, n_fwd), (1, n_bwd)):
            p, t = p0, t0
            for k in range(1, n + 1):
                p = p + dy.get_forward_backward_scene_flow(p.reshape(M, 1, 3), t)[d].reshape(M, 3)
                if rt == "contract":
                    p = torch.clamp(p, min=LO, max=HI)
                t = t + dt if d == 0 else t - dt
                pts[n_bwd + k if d == 0 else n_bwd - k] = p
        out = {"pts": torch.stack(pts, 1)}
        if cams is not None:
            pix, disp = [], []
            for k in range(K):
                c2w = cams[k][None].expand(M, 3, 4)
                if rt == "ndc":
                    a, b = rodynrf.render_single_3d_point(H, W, focal, c2w, pts[k])
                else:
                    a, b = rodynrf.render_3d_point(H, W, focal, c2w, torch.ones(M, 1, device=DEV), pts[k].reshape(M, 1, 3),
                                                   torch.zeros(M, 6, device=DEV), "contract")
                pix.append(a)
                disp.append(b[:, 0])
            out["pix"], out["disp"] = torch.stack(pix, 1), torch.stack(disp, 1)
    return out


def native(dy, p0, t0, n_fwd, n_bwd, rt, with_cams=True):
    rodynrf = _util.rodynrf()
    cams, focal, H, W = cameras()
    K = n_bwd + 1 + n_fwd
    if not with_cams:
        return rodynrf.track_points(dy, p0, t0, n_fwd, n_bwd, T_VIDEO, ray_type=rt)
    return rodynrf.track_points(dy, p0, t0, n_fwd, n_bwd, T_VIDEO, cameras=cams[:K], focal=focal, H=H, W=W, ray_type=rt)


# ---- 1 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("rt", ["ndc", "contract"])
def test_point_single_matches_the_reference(rt):
    z, dy = fixture(), field(rt)
    p0 = torch.from_numpy(z[rt + ".p0"]).to(DEV)
    t0 = torch.from_numpy(z["t0"]).to(DEV)
    with torch.no_grad():
        got = dy.get_forward_backward_scene_flow_point_single(p0, t0)
    for name, g in zip(("pts_f", "pts_b", "sf_f", "sf_b"), got):
        assert g.shape == (p0.shape[0], 3)
        assert_close(g, z[f"{rt}.single.{name}"], f"{rt} single {name}", rtol=RTOL)


def test_point_single_gradients_are_the_scene_flow_gradients():
    z, dy = fixture(), field("ndc")
    M = int(z["meta.M"])
    t0 = torch.from_numpy(z["t0"]).to(DEV)
    g = torch.Generator().manual_seed(5)
    wts = [torch.randn(M, 3, generator=g).to(DEV) for _ in range(4)]
    params = list(dy.scene_flow_mlp.parameters())

    def grads(single):
        p = torch.from_numpy(z["ndc.p0"]).to(DEV).requires_grad_(True)
        for q in dy.parameters():
            q.grad = None
        if single:
            outs = dy.get_forward_backward_scene_flow_point_single(p, t0)
        else:
            sf_f, sf_b = dy.get_forward_backward_scene_flow(p.reshape(M, 1, 3), t0)
            sf_f, sf_b = sf_f.reshape(M, 3), sf_b.reshape(M, 3)
            outs = (p + sf_f, p + sf_b, sf_f, sf_b)
        sum((o * w).sum() for o, w in zip(outs, wts)).backward()
        return [p.grad.clone()] + [q.grad.clone() for q in params]

    a, b = grads(True), grads(False)
    assert len(a) == 9 and all(float(x.abs().max()) > 0 for x in a)
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), i
    for q in dy.parameters():
        q.grad = None


# ---- 2 -----------------------------------------------------------------------------------------
CASES2 = [(rt, M, nf, nb) for rt in ("ndc", "contract") for M in SIZES for nf, nb in STEPS]
CASES2 += [(rt, M_MULTI, 5, 3) for rt in ("ndc", "contract")]


@pytest.mark.parametrize("rt,M,n_fwd,n_bwd", CASES2, ids=[f"{a}-{b}-{c}f{d}b" for a, b, c, d in CASES2])
def test_track_points_equals_the_composition_of_public_calls(rt, M, n_fwd, n_bwd):
    dy = field(rt)
    p0, t0 = seeds(rt, M)
    cams, focal, H, W = cameras()
    K = n_bwd + 1 + n_fwd
    grid, waves, tiles = launch_geometry(M)
    assert (tiles > grid * waves) == (M == M_MULTI), "M_MULTI no longer is the case in which a wave takes a second tile"
    want = compose(dy, p0, t0, n_fwd, n_bwd, rt, cams[:K], focal, H, W)
    got = native(dy, p0, t0, n_fwd, n_bwd, rt)
    assert got.points.shape == (M, K, 3) and got.pixels.shape == (M, K, 2) and got.disp.shape == (M, K)
    assert got.frames_offset.tolist() == list(range(-n_bwd, n_fwd + 1))
    assert torch.equal(got.points[:, n_bwd], p0)
    for name, a in (("pts", got.points), ("pix", got.pixels), ("disp", got.disp)):
        assert torch.isfinite(a).all(), name
        assert torch.equal(a, want[name]), (name, float((a - want[name]).abs().max()))
    if M >= 31 and n_fwd + n_bwd > 0:   # the edge cases are in play
        if rt == "contract":
            moved = torch.cat([got.points[:, :n_bwd], got.points[:, n_bwd + 1:]], 1)
            assert bool((moved.abs() == torch.tensor(HI, device=DEV)).any()), "the step clamp does not fire"
        else:
            assert int((p0[:, 2] >= 1 - 1e-6).sum()) >= 3


# ---- 3 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("rt", ["ndc", "contract"])
def test_track_points_against_the_reference_chain(rt):
    z, dy = fixture(), field(rt)
    n_fwd, n_bwd = int(z["meta.n_fwd"]), int(z["meta.n_bwd"])
    p0 = torch.from_numpy(z[rt + ".p0"]).to(DEV)
    t0 = torch.from_numpy(z["t0"]).to(DEV)
    cams, focal, H, W = cameras()
    comp = compose(dy, p0, t0, n_fwd, n_bwd, rt, cams, focal, H, W)
    got = native(dy, p0, t0, n_fwd, n_bwd, rt)
    nat = {"pts": got.points, "pix": got.pixels, "disp": got.disp}
    names = ("pts", "pix", "disp") if rt == "ndc" else ("pts",)   # (the reference projects single points for ndc only)
    for name in names:
        ref = torch.from_numpy(z[f"{rt}.chain.{name}"]).double()
        scale = float(ref.abs().max())
        for k in range(n_bwd + 1 + n_fwd):
            steps = abs(k - n_bwd) + (0 if name == "pts" else 1)
            bound = steps * RTOL * scale
            err_c = float((comp[name][:, k].detach().cpu().double() - ref[:, k]).abs().max())
            err_n = float((nat[name][:, k].detach().cpu().double() - ref[:, k]).abs().max())
            record_margin(f"{rt} chain {name} slot {k - n_bwd:+d} composition / bound", err_c / bound if bound > 0 else err_c)
            record_margin(f"{rt} chain {name} slot {k - n_bwd:+d} native / composition", err_n / err_c if err_c > 0 else err_n)
            assert err_c <= bound, ("composition", name, k, err_c, bound)
            assert err_n <= err_c, ("native", name, k, err_n, err_c)


# ---- 4 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("rt", ["ndc", "contract"])
def test_outputs_do_not_depend_on_the_split_or_on_the_requested_outputs(rt):
    R = pkg("renderer")
    dy = field(rt)
    p0, t0 = seeds(rt, 70)
    cams, focal, H, W = cameras()
    whole = native(dy, p0, t0, 5, 3, rt)
    for sl in (slice(0, 35), slice(35, 70), slice(0, 1), slice(1, 70)):
        part = native(dy, p0[sl], t0[sl], 5, 3, rt)
        for a, b in ((part.points, whole.points), (part.pixels, whole.pixels), (part.disp, whole.disp)):
            assert torch.equal(a, b[sl]), sl
    no_cams = native(dy, p0, t0, 5, 3, rt, with_cams=False)
    assert no_cams.pixels is None and no_cams.disp is None and torch.equal(no_cams.points, whole.points)
    dt = 2.0 / (T_VIDEO - 1)
    for want, ref in ((("pts",), whole.points), (("pix",), whole.pixels), (("disp",), whole.disp)):
        b = R._track_points_raw(dy, p0, t0, 5, 3, dt, cams, focal, H, W, rt, want)
        assert list(b) == list(want) and torch.equal(b[want[0]], ref), want


# ---- 5 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("packed", [True, False], ids=["packed-image", "packs-into-workspace"])
@pytest.mark.parametrize("rt,M", [("ndc", 33), ("contract", 70)])
def test_poisoned_workspace_and_guard_bands(rt, M, packed, monkeypatch):
    R = pkg("renderer")
    F = pkg("fields")
    L = pkg()
    monkeypatch.setattr(F, "PACK_CACHE", packed)
    dy = field(rt)
    p0, t0 = seeds(rt, M)
    cams, focal, H, W = cameras()
    n_fwd, n_bwd, K, G = 5, 3, 9, 257
    ref = native(dy, p0, t0, n_fwd, n_bwd, rt)
    nan = float("nan")
    for want in (("pts", "pix", "disp"), ("pts",), ("pix",)):
        sizes = {"pts": M * K * 3, "pix": M * K * 2, "disp": M * K}
        big = torch.full((G + sum(sizes[n] + G for n in want),), nan, device=DEV)
        bufs, guards, o = {}, [(0, G)], G
        for n in want:
            bufs[n] = big[o:o + sizes[n]].view((M, K, 3) if n == "pts" else (M, K, 2) if n == "pix" else (M, K))
            o += sizes[n]
            guards.append((o, o + G))
            o += G
        ws = torch.full((int(L.lib.rdrf_track_ws_bytes(M, K)) // 4 + G,), nan, device=DEV).view(torch.uint8)
        ws_tail = ws.view(torch.float32)[-G:]
        R._track_points_raw(dy, p0, t0, n_fwd, n_bwd, 2.0 / (T_VIDEO - 1), cams, focal, H, W, rt, want, bufs=bufs,
                            ws=ws[:ws.numel() - 4 * G])
        for n, r in (("pts", ref.points), ("pix", ref.pixels), ("disp", ref.disp)):
            if n in want:
                assert torch.isfinite(bufs[n]).all(), (want, n)
                assert torch.equal(bufs[n], r), (want, n)
        for a, b in guards:
            assert bool(torch.isnan(big[a:b]).all()), (want, a)
        assert bool(torch.isnan(ws_tail).all())


# ---- 6 -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tiny_scene(rt, empty=False):
    """empty: relu density and a dynamic density head that puts out -1 everywhere -- sigma_d is exactly 0, acc_d = 0, every seed
    is its ray's far point"""
    from _gpu_util import COMMON
    rodynrf = _util.rodynrf()
    torch.manual_seed(31)
    aabb = torch.tensor([[-1.5, -1.67, -1.0], [1.5, 1.67, 1.0]]) if rt == "ndc" else torch.tensor([[-2.0] * 3, [2.0] * 3])
    kw = dict(COMMON, near_far=[0.0, 1.0] if rt == "ndc" else [0.0, 256.0], density_shift=-1.0, fea2denseAct="relu" if empty else "softplus")
    grid = [17, 19, 11]
    st = rodynrf.TensorVMSplit(aabb, grid, 12, DEV, shadingMode="MLP_Fea", fea_pe=2, **kw)
    dy = rodynrf.TensorVMSplit_TimeEmbedding(aabb, grid, 12, DEV, shadingMode="MLP_Fea_late_view", fea_pe=0, **kw)
    if empty:
        with torch.no_grad():
            dy.density_layer2.weight.zero_()
            dy.density_layer2.bias.fill_(-1.0)
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
def test_render_tracks_on_a_tiny_scene(rt):
    rodynrf = _util.rodynrf()
    st, dy, p9, focal, T, H, W, pixels = tiny_scene(rt)
    S, frame = 13, 2
    ids = pixels[:, 1] * W + pixels[:, 0] + frame * H * W
    rays = rodynrf.generate_rays(ids, p9, focal, H, W, ndc=rt == "ndc", near=1.0)
    ts = torch.full((40,), 2.0 * frame / (T - 1) - 1.0, device=DEV)
    before = rodynrf.render_rays(st, dy, rays, ts, S, rt, maps=True)
    tracks, acc_d = rodynrf.render_tracks(st, dy, p9, focal, frame, pixels, H, W, N_samples=S, ray_type=rt)
    after = rodynrf.render_rays(st, dy, rays, ts, S, rt, maps=True)
    for n in before._fields:
        assert torch.equal(getattr(before, n), getattr(after, n)), n
    assert torch.equal(acc_d, before.acc_d)
    assert tracks.points.shape == (40, T, 3) and tracks.frames_offset.tolist() == list(range(-frame, T - frame))
    for a in (tracks.points, tracks.pixels, tracks.disp):
        assert torch.isfinite(a).all()
    # the seed slot against the pixel centres, to the margin render_3d_point itself shows on these rays
    with torch.no_grad():
        xyz, z, valid = rodynrf.sampleXYZ(dy, rays, S, ray_type=rt, is_train=False)
        o_s = st(rays, ts, None, xyz, z, valid, ray_type=rt, N_samples=S)
        o_d = dy(rays, ts, None, xyz, z, valid, ray_type=rt, N_samples=S)
        outs = rodynrf.raw2outputs(o_s[6], o_s[7], o_d[6], o_d[7], o_d[9], o_d[2], o_d[8], rays, is_train=False, ray_type=rt)
        own = rodynrf.pose_to_mtx(p9)[frame][None].expand(40, 3, 4)
        pix_ref, _ = rodynrf.render_3d_point(H, W, focal, own, outs[11], o_d[3], rays, rt)
        # the seed itself: render_3d_point's first half (renderer.py:1333-1345) in torch, at the forward tolerance
        w_d, acc = outs[11], outs[11].sum(-1, keepdim=True)
        if rt == "ndc":
            far = rays[:, :3] + rays[:, 3:]
        else:
            far = rays[:, :3] + rays[:, 3:] * 256.0
            nrm = far.abs().max(-1, keepdim=True)[0]
            far = torch.where(nrm > 1.0, (2.0 - 1.0 / nrm) * (far / nrm), far)
        seed_ref = (w_d[..., None] * o_d[3]).sum(1) + (1.0 - acc) * far
    print(f"{rt}: acc_d of the seeds in [{float(acc.min()):.3g}, {float(acc.max()):.3g}]")
    assert_close(tracks.points[:, frame], seed_ref, f"{rt} render_tracks seed point", rtol=RTOL)
    assert_close(tracks.pixels[:, frame], pix_ref, f"{rt} render_tracks seed pixels vs render_3d_point", rtol=RTOL)
    centre = pixels.float() + 0.5
    err_ref = float((pix_ref - centre).abs().max())
    err = float((tracks.pixels[:, frame] - centre).abs().max())
    record_margin(f"{rt} render_3d_point vs pixel centres [pixels]", err_ref)
    record_margin(f"{rt} render_tracks seed slot vs pixel centres [pixels]", err)
    print(f"{rt}: render_3d_point {err_ref:.3e} px, render_tracks seed slot {err:.3e} px off the pixel centres")
    assert err <= err_ref, (err, err_ref)
    # span clips at frame 0 and at frame T - 1
    for fr, span, offs in ((0, 2, [0, 1, 2]), (T - 1, 2, [-2, -1, 0]), (1, 3, [-1, 0, 1, 2, 3]), (3, (1, 0), [-1, 0]),
                           (T - 1, None, list(range(-(T - 1), 1)))):
        tr, acc = rodynrf.render_tracks(st, dy, p9, focal, fr, pixels, H, W, span=span, N_samples=S, ray_type=rt)
        assert tr.frames_offset.tolist() == offs and tr.points.shape == (40, len(offs), 3) and acc.shape == (40,), (fr, span)
        assert tr.pixels.shape == (40, len(offs), 2) and torch.isfinite(tr.pixels).all()
    # a clipped track is the same track, cut
    full, _ = rodynrf.render_tracks(st, dy, p9, focal, frame, pixels, H, W, N_samples=S, ray_type=rt)
    cut, _ = rodynrf.render_tracks(st, dy, p9, focal, frame, pixels, H, W, span=1, N_samples=S, ray_type=rt)
    assert torch.equal(cut.points, full.points[:, frame - 1:frame + 2]) and torch.equal(cut.pixels, full.pixels[:, frame - 1:frame + 2])


@pytest.mark.parametrize("rt", ["ndc", "contract"])
def test_render_tracks_seeds_in_empty_space_are_the_far_points(rt):
    """the (1 - acc_d) far leg of the seed, which the scene above (acc_d = 1 on every ray) leaves at 0"""
    rodynrf = _util.rodynrf()
    st, dy, p9, focal, T, H, W, pixels = tiny_scene(rt, True)
    S, frame = 13, 3
    tracks, acc_d = rodynrf.render_tracks(st, dy, p9, focal, frame, pixels, H, W, span=1, N_samples=S, ray_type=rt)
    assert bool((acc_d == 0).all())
    ids = pixels[:, 1] * W + pixels[:, 0] + frame * H * W
    rays = rodynrf.generate_rays(ids, p9, focal, H, W, ndc=rt == "ndc", near=1.0)
    if rt == "ndc":
        far = rays[:, :3] + rays[:, 3:]
    else:
        far = rays[:, :3] + rays[:, 3:] * 256.0
        nrm = far.abs().max(-1, keepdim=True)[0]
        assert bool((nrm > 1.0).all())
        far = (2.0 - 1.0 / nrm) * (far / nrm)
    assert_close(tracks.points[:, 1], far, f"{rt} render_tracks seed point, empty space", rtol=RTOL)
    own = rodynrf.pose_to_mtx(p9)[frame][None].expand(40, 3, 4)
    pix_ref, _ = rodynrf.render_3d_point(H, W, focal, own, torch.zeros(40, S, device=DEV), torch.zeros(40, S, 3, device=DEV), rays, rt)
    assert_close(tracks.pixels[:, 1], pix_ref, f"{rt} render_tracks seed pixels vs render_3d_point, empty space", rtol=RTOL)


# ---- 7 -----------------------------------------------------------------------------------------
def det_case():
    """what both libraries compute (tests/_det_child.py case): the (5, 3) tracks of test 2 at M = 70"""
    out = {}
    for rt in ("ndc", "contract"):
        p0, t0 = seeds(rt, 70)
        tr = native(field(rt), p0, t0, 5, 3, rt)
        out.update({f"{rt}.pts": tr.points, f"{rt}.pix": tr.pixels, f"{rt}.disp": tr.disp})
    return out


def test_deterministic_library_gives_the_same_bits(tmp_path):
    ours = det_case()
    assert_same_dict(run_twin(tmp_path, [CHILD, "case", "test_gpu_tracks"], det=True), ours)
