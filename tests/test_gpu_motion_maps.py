"""Motion maps of the native evaluation render (rdrf_render_motion_fwd, rdrf_flow_to_image) on the GPU: parity with the
reference's own per-frame chain (tests/golden/motion_*.npz, make_golden_motion.py), bit-stability across render modes,
chunkings, repeats and map subsets, the colour maps left untouched, the composition of the public calls at a real shape,
edge shapes, and the flow pictures against flow_viz.flow_to_image."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from _gpu_util import fields_from_case
from _twin import CHILD, assert_same_dict, run_twin, same_bits
from _util import GOLDEN, assert_close, pkg

pytestmark = pytest.mark.gpu

MOTION = ("flow_f", "flow_b", "flow_s_f", "flow_s_b", "delta_xyz")
CASES = ["motion_ndc", "motion_contract"]
CANARY = 12345.0


def _case(name):
    g, st, dy, _ = fields_from_case(name)
    dev = "cuda"
    t = lambda k: torch.from_numpy(np.array(g[k])).to(dev)
    cams = dict(H=int(g["meta.H"]), W=int(g["meta.W"]), focal=float(g["focal"]), c2w_f=t("c2w_f"), c2w_b=t("c2w_b"))
    return g, st, dy, t("rays"), t("ts"), int(g["meta.S"]), str(g["meta.ray_type"]), cams


def _native(st, dy, rays, ts, S, rt, cams, want=MOTION, mode="auto", first=0, maps=None):
    """rdrf_render_motion_fwd with caller-owned buffers: all five motion buffers exist and are pre-filled with a canary, only
    the pointers of `want` are passed.  Returns (dict of the five buffers, dict of the requested RenderMaps buffers)."""
    L = pkg()
    F = pkg("fields")
    R = pkg("renderer")
    N, dev = rays.shape[0], rays.device
    bufs = {n: torch.full((N, 3) if n == "delta_xyz" else (N, 2), CANARY, device=dev) for n in MOTION}
    MM = L.MotionMapsC(*[bufs[n].data_ptr() if n in want else None for n in MOTION])
    focal = torch.full((1,), float(cams["focal"]), device=dev)
    cf, cb = cams["c2w_f"].contiguous(), cams["c2w_b"].contiguous()
    MC = L.MotionCamsC(cams["H"], cams["W"], focal.data_ptr(), cf.data_ptr(), cb.data_ptr(), int(first))
    mbufs = R._alloc_maps(maps, N, dev) if maps else {}
    M = R._maps_struct(mbufs)
    ws = L.workspace(dev, int(L.lib.rdrf_render_motion_workspace_bytes(N, S)))
    ps_list, pd_list = st._param_list(), dy._param_list()
    PS, PD = F._static_struct(ps_list), F._dynamic_struct(pd_list)
    F._attach_packed(st, PS, ps_list, False, False)
    F._attach_packed(dy, PD, pd_list, False, True)
    cs, cd = F._cfg_struct(st, rt), F._cfg_struct(dy, rt)
    near, far = dy.near_far
    L.check(L.lib.rdrf_render_motion_fwd(C.byref(PS), C.byref(cs), C.byref(PD), C.byref(cd), L.ptr(rays), L.ptr(ts), N, S,
                                         near, far, L.RENDER_MODES[mode], C.byref(M), C.byref(MC), C.byref(MM), L.ptr(ws),
                                         ws.numel(), L.stream_of(rays)), "rdrf_render_motion_fwd")
    torch.cuda.synchronize()
    return bufs, mbufs


def _composition(st, dy, rays, ts, S, rt, cams, first=0):
    """the motion maps from the public calls that exist without the native path: forward x 2, raw2outputs,
    get_forward_backward_scene_flow, induce_flow x 4, a torch sum for delta_xyz (the order of renderer.py:405-537)"""
    import rodynrf
    with torch.no_grad():
        N, dev = rays.shape[0], rays.device
        H, W, f = cams["H"], cams["W"], cams["focal"]
        xyz, z, valid = rodynrf.sampleXYZ(dy, rays, S, ray_type=rt, is_train=False)
        o_s = st(rays, ts, None, xyz, z, valid, ray_type=rt, N_samples=S)
        o_d = dy(rays, ts, None, xyz, z, valid, ray_type=rt, N_samples=S)
        outs = rodynrf.raw2outputs(o_s[6], o_s[7], o_d[6], o_d[7], o_d[9], o_d[2], o_d[8], rays, is_train=False, ray_type=rt)
        w_s, w_d = outs[7], outs[11]
        sf_f, sf_b = dy.get_forward_backward_scene_flow(o_d[3], ts)
        pix = torch.arange(N, device=dev) + first
        p2d = torch.stack([pix % W, (pix // W) % H], -1).float()
        tile = lambda p: p[None].expand(N, 3, 4).contiguous()
        pf, pb = tile(cams["c2w_f"]), tile(cams["c2w_b"])
        return dict(
            flow_f=rodynrf.induce_flow(H, W, f, pf, w_d, o_d[3] + sf_f, p2d, rays, rt)[0],
            flow_b=rodynrf.induce_flow(H, W, f, pb, w_d, o_d[3] + sf_b, p2d, rays, rt)[0],
            flow_s_f=rodynrf.induce_flow(H, W, f, pf, w_s, o_s[3], p2d, rays, rt)[0],
            flow_s_b=rodynrf.induce_flow(H, W, f, pb, w_s, o_s[3], p2d, rays, rt)[0],
            delta_xyz=torch.sum(w_d[..., None] * (o_d[5] - xyz), 1), w_d=w_d)


# ---- 1. reference parity ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["auto", "sequence", "fused"])
@pytest.mark.parametrize("case", CASES)
def test_motion_maps_match_the_reference(case, mode):
    import rodynrf
    g, st, dy, rays, ts, S, rt, cams = _case(case)
    (rgb, depth), mm = rodynrf.render_rays(st, dy, rays, ts, S, ray_type=rt, mode=mode, motion=cams)
    for k in MOTION:
        err = float((getattr(mm, k).cpu().double() - torch.from_numpy(g["out." + k]).double()).abs().max())
        print(f"{case} {mode} {k}: max err {err:.3e} of max|ref| {float(np.abs(g['out.' + k]).max()):.3e}")
    for k in MOTION:
        assert_close(getattr(mm, k), g["out." + k], f"{case}.{mode}.{k}", rtol=1e-4)
    assert_close(rgb, np.clip(g["out.rgb"], 0.0, 1.0), f"{case}.{mode}.rgb", rtol=1e-4)
    assert_close(depth, g["out.depth"], f"{case}.{mode}.depth", rtol=1e-4)


# ---- 2. same bits everywhere ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_motion_maps_same_bits_everywhere(case):
    import rodynrf
    g, st, dy, rays, ts, S, rt, cams = _case(case)
    N = rays.shape[0]
    base, _ = _native(st, dy, rays, ts, S, rt, cams)
    assert all(torch.isfinite(base[k]).all() and not (base[k] == CANARY).any() for k in MOTION)
    for mode in ("sequence", "fused"):                       # the three modes
        got, _ = _native(st, dy, rays, ts, S, rt, cams, mode=mode)
        for k in MOTION:
            assert same_bits(got[k], base[k]), (mode, k)
    for rep in range(3):                                     # three repeats
        got, _ = _native(st, dy, rays, ts, S, rt, cams)
        for k in MOTION:
            assert same_bits(got[k], base[k]), (rep, k)
    # whole image vs chunks with first_pixel: multiples of 32 rays (96), of S (40), of neither (37, 100), through the
    # public call and through render_frame's chunk loop
    for chunk in (96, S, 37, 100):
        parts = [rodynrf.render_rays(st, dy, rays[c0:c0 + chunk], ts[c0:c0 + chunk], S, ray_type=rt,
                                     motion=dict(cams, first_pixel=c0))[1] for c0 in range(0, N, chunk)]
        for k in MOTION:
            assert same_bits(torch.cat([getattr(p, k) for p in parts]), base[k]), (chunk, k)
    R = pkg("renderer")
    _, img = R._render_image(st, dy, rays, ts, cams["H"], cams["W"], S, rt, 100, False, dict(cams))
    for k in MOTION:
        assert same_bits(getattr(img, k).reshape(N, -1), base[k]), k
    # any subset gives the bits of the full request; an unrequested buffer keeps its canary
    subsets = [(k,) for k in MOTION] + [("flow_f", "flow_s_b"), ("flow_b", "delta_xyz"), ("flow_s_f", "flow_s_b", "delta_xyz")]
    for want in subsets:
        got, _ = _native(st, dy, rays, ts, S, rt, cams, want=want)
        for k in MOTION:
            if k in want:
                assert same_bits(got[k], base[k]), (want, k)
            else:
                assert bool((got[k] == CANARY).all()), (want, k)
    part = rodynrf.render_rays(st, dy, rays, ts, S, ray_type=rt, motion=dict(cams, maps=("flow_b",)))[1]
    assert same_bits(part.flow_b, base["flow_b"]) and part.flow_f is None and part.delta_xyz is None


def det_case():
    """what both libraries compute (tests/_det_child.py case): the five motion maps of motion_ndc"""
    import rodynrf
    g, st, dy, rays, ts, S, rt, cams = _case("motion_ndc")
    mm = rodynrf.render_rays(st, dy, rays, ts, S, ray_type=rt, motion=cams)[1]
    return {k: getattr(mm, k) for k in MOTION}


def test_motion_maps_same_bits_in_the_deterministic_library(tmp_path):
    """librodynrf_det.so in a child process (the library is chosen at import) writes the bits of the product library"""
    out = {det: run_twin(tmp_path, [CHILD, "case", "test_gpu_motion_maps"], det=det) for det in (False, True)}
    assert sorted(out[False]) == sorted(MOTION)
    assert_same_dict(out[True], out[False])


# ---- 3. the existing maps keep their bits -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_render_maps_unchanged_by_motion(case):
    import rodynrf
    g, st, dy, rays, ts, S, rt, cams = _case(case)
    for mode in ("auto", "fused"):
        ref = rodynrf.render_rays(st, dy, rays, ts, S, ray_type=rt, mode=mode, maps=True)
        got, mm = rodynrf.render_rays(st, dy, rays, ts, S, ray_type=rt, mode=mode, maps=True, motion=cams)
        for k in rodynrf.RenderMaps._fields:
            assert same_bits(getattr(got, k), getattr(ref, k)), (mode, k)
        rgb, depth = rodynrf.render_rays(st, dy, rays, ts, S, ray_type=rt, mode=mode)
        (rgb2, depth2), _ = rodynrf.render_rays(st, dy, rays, ts, S, ray_type=rt, mode=mode, motion=cams)
        assert same_bits(rgb, rgb2) and same_bits(depth, depth2), mode
        sub, _ = rodynrf.render_rays(st, dy, rays, ts, S, ray_type=rt, mode=mode, maps=("depth_d", "blending"), motion=cams)
        assert same_bits(sub.depth_d, ref.depth_d) and same_bits(sub.blending, ref.blending) and sub.rgb is None


# ---- 4. composition at a real shape -------------------------------------------------------------------------------------
def test_motion_maps_match_the_composition_at_stage0():
    """Stage-0 frame (240 x 135, grid [141,157,94], S = 115, the seeded initialiser, scene-flow head scaled until the dynamic
    flows leave the static ones by a pixel): the native maps against the composition of the public calls, rtol 1e-4 of
    max|ref| over the rays whose composition flows are moderate (|flow| < 1e4: more than 90 % of them), the others finite.
    Measured on an MI355X: every ray kept; max error / max|ref| 3.4e-6 (flow_f), 4.5e-6 (flow_b), 7.6e-5 (flow_s_f),
    2.3e-5 (flow_s_b), 2.0e-7 (delta_xyz).  The static flows are the tight ones: the projected pixel coordinate is up to 240,
    two of its fp32 ulps are 3e-5 px, and the static forward flow itself is at most half a pixel on this frame."""
    import rodynrf
    S_ = pkg("step")
    dev = torch.device("cuda", 0)
    cfg = S_.scene_config("nvidia", "stage0")
    torch.manual_seed(7)
    tr = S_.Trainer(cfg, dev)
    H, W, S, rt, frame = cfg["H"], cfg["W"], cfg["n_samples"], cfg["ray_type"], 3
    assert (W, H, S) == (240, 135, 115)
    poses, focal = tr.pose_table().detach(), tr.focal()
    focal = float(focal.detach()) if torch.is_tensor(focal) else float(focal)
    mtx = rodynrf.pose_to_mtx(poses.float())
    T = poses.shape[0]
    cams = dict(H=H, W=W, focal=focal, c2w_f=mtx[min(frame + 1, T - 1)].contiguous(), c2w_b=mtx[max(frame - 1, 0)].contiguous())
    ids = torch.arange(H * W, device=dev) + frame * H * W
    rays = rodynrf.generate_rays(ids, poses, focal, H, W, ndc=rt == "ndc", near=1.0).detach()
    ts = torch.full((H * W,), 2.0 * frame / max(T - 1, 1) - 1.0, device=dev)
    with torch.no_grad():
        for _ in range(40):
            ref = _composition(tr.st, tr.dy, rays, ts, S, rt, cams)
            gap = min(float((ref["flow_f"] - ref["flow_s_f"]).abs().median()), float((ref["flow_b"] - ref["flow_s_b"]).abs().median()))
            if gap >= 1.0:
                break
            tr.dy.scene_flow_mlp[6].weight *= 2.0
            tr.dy.scene_flow_mlp[6].bias *= 2.0
    assert gap >= 1.0, gap
    (_, _), mm = rodynrf.render_frame(tr.st, tr.dy, poses, focal, frame, H, W, N_samples=S, ray_type=rt, motion=True)
    flows = torch.stack([ref[k] for k in MOTION[:4]], 0)
    ok = (flows.abs().amax((0, 2)) < 1e4).cpu()
    print(f"stage0: kept {float(ok.float().mean()):.4f} of the rays, gap {gap:.2f} px, "
          f"rays with sum weights_d > 0.1: {float((ref['w_d'].sum(-1) > 0.1).float().mean()):.3f}")
    assert float(ok.float().mean()) > 0.9
    for k in MOTION:
        a, b = getattr(mm, k).reshape(H * W, -1).cpu(), ref[k].cpu()
        assert torch.isfinite(a).all(), k
        m = ok[:, None].expand_as(a)
        print(f"stage0 {k}: max err {float((a - b)[m].abs().max()):.3e} of max|ref| {float(b[m].abs().max()):.3e}")
    for k in MOTION:
        a, b = getattr(mm, k).reshape(H * W, -1).cpu(), ref[k].cpu()
        assert_close(a, b, "stage0." + k, rtol=1e-4, mask=ok[:, None].expand_as(a))


# ---- 5. edges -----------------------------------------------------------------------------------------------------------
def test_motion_maps_first_and_last_frame():
    """frame 0 / T - 1: the missing neighbour is the frame's own camera (renderer.py:386-387)"""
    import rodynrf
    g, st, dy, _, _, S, rt, cams = _case("motion_ndc")
    dev, H, W, T = "cuda", cams["H"], cams["W"], 5
    gen = torch.Generator().manual_seed(11)
    p9 = torch.zeros(T, 9)
    p9[:, 0] = 1
    p9[:, 4] = 1
    p9 = (p9 + 0.03 * torch.randn(T, 9, generator=gen)).to(dev)
    mtx = rodynrf.pose_to_mtx(p9)
    for frame in (0, T - 1, 2):
        (_, _), mm = rodynrf.render_frame(st, dy, p9, cams["focal"], frame, H, W, N_samples=S, ray_type=rt, motion=True)
        ids = torch.arange(H * W, device=dev) + frame * H * W
        rays = rodynrf.generate_rays(ids, p9, cams["focal"], H, W, ndc=True, near=1.0)
        ts = torch.full((H * W,), 2.0 * frame / (T - 1) - 1.0, device=dev)
        c = dict(cams, c2w_f=mtx[min(frame + 1, T - 1)].contiguous(), c2w_b=mtx[max(frame - 1, 0)].contiguous())
        ref = _composition(st, dy, rays, ts, S, rt, c)
        for k in MOTION:
            assert getattr(mm, k).shape == (H, W, 3 if k == "delta_xyz" else 2)
            assert_close(getattr(mm, k).reshape(H * W, -1), ref[k], f"frame{frame}.{k}", rtol=1e-4)
        own = _composition(st, dy, rays, ts, S, rt, dict(cams, c2w_f=mtx[frame].contiguous(), c2w_b=mtx[frame].contiguous()))
        if frame == 0:
            assert_close(mm.flow_s_b.reshape(H * W, 2), own["flow_s_b"], "frame0.own_pose", rtol=1e-4)
        if frame == T - 1:
            assert_close(mm.flow_s_f.reshape(H * W, 2), own["flow_s_f"], "last.own_pose", rtol=1e-4)


@pytest.mark.parametrize("case,N,S", [("motion_ndc", 45, 13), ("motion_contract", 45, 13), ("motion_ndc", 77, 115)])
def test_motion_maps_edge_shapes(case, N, S):
    """N not a multiple of 32, S = 13 (one partial tile) and S = 115 (a partial fourth tile); ndc: ray 0 misses the box, so
    all its weights_d are exactly 0 and its maps are the far point's"""
    import rodynrf
    g, st, dy, rays, ts, _, rt, cams = _case(case)
    rays, ts = rays[:N].clone(), ts[:N].clone()
    if rt == "ndc":
        rays[0, :3] = torch.tensor([5.0, 5.0, -1.0], device=rays.device)
    ref = _composition(st, dy, rays, ts, S, rt, cams, first=7)
    if rt == "ndc":
        assert float(ref["w_d"][0].abs().max()) == 0.0
    for mode in ("auto", "fused"):
        _, mm = rodynrf.render_rays(st, dy, rays, ts, S, ray_type=rt, mode=mode, motion=dict(cams, first_pixel=7))
        for k in MOTION:
            assert torch.isfinite(getattr(mm, k)).all(), k
            assert_close(getattr(mm, k), ref[k], f"{case}.{N}x{S}.{mode}.{k}", rtol=1e-4)
        if rt == "ndc":
            assert float(mm.delta_xyz[0].abs().max()) == 0.0
            assert_close(mm.flow_f[0], ref["flow_f"][0], "empty ray", rtol=1e-4)


# ---- 6. flow colours ------------------------------------------------------------------------------------------------------
def _flow_image_f64(flow):
    """flow_viz.flow_to_image's formula (flow_viz.py:23-136) evaluated in float64 throughout on a finite flow"""
    seg = (15, 6, 4, 11, 13, 6)
    wheel = np.zeros((55, 3))
    full, var = (0, 1, 1, 2, 2, 0), (1, 0, 2, 1, 0, 2)
    col = 0
    for i, n in enumerate(seg):
        ramp = np.floor(255 * np.arange(n) / n)
        wheel[col:col + n, full[i]] = 255
        wheel[col:col + n, var[i]] = 255 - ramp if i % 2 else ramp
        col += n
    f = flow.astype(np.float64)
    u, v = f[..., 0], f[..., 1]
    rad_max = np.sqrt(u * u + v * v).max()
    u, v = u / (rad_max + 1e-5), v / (rad_max + 1e-5)
    rad = np.sqrt(u * u + v * v)
    fk = (np.arctan2(-v, -u) / np.pi + 1) / 2 * 54
    k0 = np.floor(fk).astype(np.int64)
    k1 = np.where(k0 + 1 == 55, 0, k0 + 1)
    fr = fk - k0
    img = np.zeros(flow.shape[:2] + (3,), np.uint8)
    for c in range(3):
        cc = (1 - fr) * wheel[k0, c] / 255.0 + fr * wheel[k1, c] / 255.0
        cc = np.where(rad <= 1, 1 - rad * (1 - cc), cc * 0.75)
        img[..., c] = np.floor(255 * cc)
    return img


@pytest.mark.parametrize("case", CASES)
def test_flow_to_image_matches_flow_viz(case):
    import rodynrf
    g = np.load(os.path.join(GOLDEN, case + ".npz"))
    H, W = int(g["meta.H"]), int(g["meta.W"])
    total = 0
    for k in MOTION[:4]:
        flow = g["out." + k].reshape(H, W, 2)
        ref = g["viz." + k]
        dflow = torch.from_numpy(flow.copy()).cuda()
        got = rodynrf.flow_to_image(dflow)
        assert got.dtype == torch.uint8 and got.shape == (H, W, 3)
        assert torch.equal(dflow.cpu(), torch.from_numpy(flow)), "the input flow is not modified"
        diff = np.abs(got.cpu().numpy().astype(np.int32) - ref.astype(np.int32))
        bound = int((_flow_image_f64(flow) != ref).sum())
        print(f"{case} {k}: {int((diff > 0).sum())} of {diff.size} channel values differ from flow_viz "
              f"(flow_viz vs its fp64 evaluation: {bound})")
        assert diff.max() <= 1, (k, int(diff.max()))
        assert int((diff > 0).sum()) <= bound, (k, int((diff > 0).sum()), bound)
        total += int((diff > 0).sum())
    print(f"{case}: {total} differing channel values in all four pictures")
    for tag in ("inf", "nan"):
        got = rodynrf.flow_to_image(torch.from_numpy(g[f"viz_{tag}.flow"].copy()).cuda()).cpu().numpy()
        assert np.array_equal(got, g[f"viz_{tag}.image"]), tag
    got = rodynrf.flow_to_image(torch.zeros(H, W, 2, device="cuda")).cpu().numpy()
    assert np.array_equal(got, g["viz_zero.image"])
