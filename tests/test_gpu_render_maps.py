"""GPU: the evaluation path -- decomposed maps of the native render (rdrf_render_maps_fwd / rdrf_render_chunks_maps_fwd),
rays of arbitrary cameras (rdrf_camera_rays), render_view / render_path and the device SSIM (rdrf_ssim) -- against the
reference-generated compositor outputs, the training pipeline's own forward + raw2outputs (bit for bit), float64
restatements of dataLoader/ray_utils.py and utils.py:98-151, and the existing render entry points."""
import numpy as np
import pytest
import torch

from _util import CASES, assert_close, load_case, pkg

pytestmark = pytest.mark.gpu

# RenderMaps field -> golden compositor key (renderer.py:173-315 output names)
GOLDEN_KEY = {"rgb": "rgb_map_full", "depth": "depth_map_full", "acc": "acc_map_full", "rgb_s": "rgb_map_s",
              "depth_s": "depth_map_s", "acc_s": "acc_map_s", "rgb_d": "rgb_map_d", "depth_d": "depth_map_d",
              "acc_d": "acc_map_d", "blending": "dynamicness_map"}
# RenderMaps field -> index in raw2outputs' 13-tuple
OUT_INDEX = {"rgb": 0, "depth": 1, "acc": 2, "rgb_s": 4, "depth_s": 5, "acc_s": 6, "rgb_d": 8, "depth_d": 9, "acc_d": 10,
             "blending": 12}
# the golden z of the jittered cases is not the eval sampler's: only the jitter-free cases are eval renders
EVAL_CASES = [c for c in CASES if "jitter" not in load_case(c)[0]]


def _maps_equal(a, b, names=None):
    for n in names or a._fields:
        assert torch.equal(getattr(a, n), getattr(b, n)), n


@pytest.mark.parametrize("case", EVAL_CASES)
def test_render_maps_match_reference_compositor_outputs(case):
    import rodynrf
    from _gpu_util import fields_from_case
    g, st, dy, _ = fields_from_case(case)
    rt = str(g["meta.ray_type"])
    rays, ts = torch.from_numpy(g["rays"]).cuda(), torch.from_numpy(g["ts"]).cuda()
    m = rodynrf.render_rays(st, dy, rays, ts, N_samples=g["z"].shape[1], ray_type=rt, maps=True)
    assert isinstance(m, rodynrf.RenderMaps)
    for n, k in GOLDEN_KEY.items():
        atol = 256.0 * 2.0 ** -22 if (rt == "contract" and n.startswith("depth")) else 0.0
        assert_close(getattr(m, n), g["ce." + k], f"{case} {n}", atol=atol)


@pytest.mark.parametrize("rt", ["ndc", "contract"])
@pytest.mark.parametrize("N,S", [(1, 1), (7, 13), (513, 115), (2100, 37)])
def test_render_maps_are_bit_identical_to_the_training_pipeline(rt, N, S):
    """fields' forward under no_grad, then raw2outputs(is_train=False): the same arithmetic on the same samples"""
    import rodynrf
    from _gpu_util import fields_from_case, make_rays
    if rt == "contract" and S == 1:
        S = 2   # the contracted sampler needs two samples (an inner and an outer one, models/tensorBase.py:524-559)
    g, st, dy, _ = fields_from_case("ndc_relu" if rt == "ndc" else "contract_relu_te")
    rays, ts = (t.cuda() for t in make_rays(N, 17, rt))
    m = rodynrf.render_rays(st, dy, rays, ts, N_samples=S, ray_type=rt, maps=True)
    with torch.no_grad():
        xyz, z, valid = rodynrf.sampleXYZ(dy, rays, S, ray_type=rt, is_train=False)
        o_s = st(rays, ts, None, xyz, z, valid, is_train=False, ray_type=rt, N_samples=S)
        o_d = dy(rays, ts, None, xyz, z, valid, is_train=False, ray_type=rt, N_samples=S)
        outs = rodynrf.raw2outputs(o_s[6], o_s[7], o_d[6], o_d[7], o_d[9], o_d[2], o_d[8], rays, is_train=False,
                                   ray_type=rt)
    for n, i in OUT_INDEX.items():
        assert torch.equal(getattr(m, n), outs[i]), n


@pytest.mark.parametrize("case,N,S", [("ndc_relu", 777, 115), ("contract_relu_te", 2100, 37)])
def test_render_maps_agree_with_every_render_path(case, N, S):
    """rgb / depth of the maps call = render_rays in all three modes; the fused launch gives all ten maps of the
    sequence; render_chunks(maps=True) -- one stream (chunk by chunk) and four (coalesced), a ragged last chunk --
    equals the whole batch; a requested subset keeps its bits."""
    import rodynrf
    from _gpu_util import fields_from_case, make_rays
    g, st, dy, _ = fields_from_case(case)
    rt = str(g["meta.ray_type"])
    rays, ts = (t.cuda() for t in make_rays(N, 23, rt))
    seq = rodynrf.render_rays(st, dy, rays, ts, N_samples=S, ray_type=rt, mode="sequence", maps=True)
    for mode in ("auto", "sequence", "fused"):
        rgb, depth = rodynrf.render_rays(st, dy, rays, ts, N_samples=S, ray_type=rt, mode=mode)
        assert torch.equal(seq.rgb, rgb) and torch.equal(seq.depth, depth), mode
        _maps_equal(seq, rodynrf.render_rays(st, dy, rays, ts, N_samples=S, ray_type=rt, mode=mode, maps=True))
    for streams in (1, 4):
        ch = rodynrf.render_chunks(st, dy, rays, ts, 256, N_samples=S, ray_type=rt, streams=streams, maps=True)
        torch.cuda.synchronize()
        _maps_equal(seq, ch)
        rgb, depth = rodynrf.render_chunks(st, dy, rays, ts, 256, N_samples=S, ray_type=rt, streams=streams)
        torch.cuda.synchronize()
        assert torch.equal(seq.rgb, rgb) and torch.equal(seq.depth, depth)
    one = rodynrf.render_chunks(st, dy, rays, ts, 4 * N, N_samples=S, ray_type=rt, streams=4, maps=True)
    _maps_equal(seq, one)
    sub = ("rgb_s", "depth_d", "blending")
    for mode in ("sequence", "fused"):
        part = rodynrf.render_rays(st, dy, rays, ts, N_samples=S, ray_type=rt, mode=mode, maps=sub)
        _maps_equal(seq, part, sub)
        assert all(getattr(part, n) is None for n in part._fields if n not in sub)
    part = rodynrf.render_chunks(st, dy, rays, ts, 300, N_samples=S, ray_type=rt, streams=4, maps=sub)
    torch.cuda.synchronize()
    _maps_equal(seq, part, sub)


def test_every_entry_point_of_the_family_gives_the_bits_of_the_maps_sequence():
    """70 rays (no multiple of 4, 16, 32 or 64) x 37 samples (no multiple of 32) through every no-grad render entry point:
    rgb and depth equal those of rdrf_render_maps_fwd in sequence mode bit for bit.  Chunks of 32 (a partial last chunk) on no
    side stream and on two (the workspace of two streams lets chunks coalesce); the masked render with all-ones masks; of the
    motion and track-seed calls, their render maps.  rdrf_render_world_fwd takes world-space rays only and the sequence of
    rdrf_render_maps_fwd refuses them, so the world fields are held to that entry point's own sequence mode, and so is the
    masked render on world rays."""
    import rodynrf
    import test_gpu_masked_render as MR
    import ctypes as C
    R = pkg("renderer")
    L = pkg()
    N, S = 70, 37

    def family(case, world):
        st, dy, rt = MR.fields(case)
        rays, ts = MR.make_rays(case, N)
        ref = rodynrf.render_rays(st, dy, rays, ts, S, ray_type=rt, mode="sequence", maps=True)
        assert torch.isfinite(ref.rgb).all() and float(ref.acc.max()) > 0.1, case

        def same(got, what):
            rgb, depth = (got.rgb, got.depth) if isinstance(got, rodynrf.RenderMaps) else got
            torch.cuda.synchronize()
            assert torch.equal(rgb, ref.rgb) and torch.equal(depth, ref.depth), f"{case}: {what}"

        for mode in ("auto", "sequence", "fused"):   # rdrf_render_fwd / _sequence_fwd / _fused_fwd; world: rdrf_render_world_fwd
            same(rodynrf.render_rays(st, dy, rays, ts, S, ray_type=rt, mode=mode), mode)
            same(rodynrf.render_rays(st, dy, rays, ts, S, ray_type=rt, mode=mode, maps=True), mode + " maps")
        for streams in (0, 2):   # rdrf_render_chunks_fwd / _chunks_maps_fwd
            same(rodynrf.render_chunks(st, dy, rays, ts, 32, S, ray_type=rt, streams=streams), f"chunks, {streams} streams")
            same(rodynrf.render_chunks(st, dy, rays, ts, 32, S, ray_type=rt, streams=streams, maps=True), f"chunk maps, {streams} streams")
        lo, hi = dy.aabb.detach().cpu()
        big = torch.stack([lo - 0.05 * (hi - lo), hi + 0.05 * (hi - lo)])
        ones = (MR.make_mask("ones", st, box=big), MR.make_mask("ones", dy, box=big))
        same(rodynrf.render_rays(st, dy, rays, ts, S, ray_type=rt, maps=True, alpha_masks=ones), "masked")   # rdrf_render_masked_fwd
        if world:
            return
        eye = torch.eye(4)[:3]
        for mode in ("sequence", "fused"):   # rdrf_render_motion_fwd
            m, _ = rodynrf.render_rays(st, dy, rays, ts, S, ray_type=rt, mode=mode, maps=True,
                                       motion=dict(H=7, W=10, focal=10.0, c2w_f=eye, c2w_b=eye))
            same(m, "motion " + mode)
        bufs, seeds = R._alloc_maps(("rgb", "depth"), N, rays.device), torch.empty(N, 3, device=rays.device)   # rdrf_render_track_seeds_fwd
        ws = L.workspace(rays.device, L.lib.rdrf_render_motion_workspace_bytes(N, S))
        PS, cs, PD, cd = R.render_structs(st, dy, rt)
        near, far = dy.near_far
        Mp = R._maps_struct(bufs)
        L.check(L.lib.rdrf_render_track_seeds_fwd(C.byref(PS), C.byref(cs), C.byref(PD), C.byref(cd), L.ptr(rays), L.ptr(ts), N, S, near,
                                                  far, C.byref(Mp), L.ptr(seeds), L.ptr(ws), ws.numel(), L.stream_of(rays)),
                "rdrf_render_track_seeds_fwd")
        same((bufs["rgb"], bufs["depth"]), "track seeds")
        assert torch.isfinite(seeds).all()

    family("ndc_relu", False)
    family("world", True)


def _camera_rays_f64(c2w, focal, H, W, ndc, near=1.0):
    """dataLoader/ray_utils.py: get_ray_directions_blender -> get_rays -> ndc_rays_blender, float64, per camera"""
    out = []
    for b in range(c2w.shape[0]):
        f = float(focal[b])
        j, i = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
        i, j = i + 0.5, j + 0.5
        dirs = torch.stack([(i - W / 2) / f, -(j - H / 2) / f, -torch.ones_like(i)], -1)
        M = c2w[b].double()
        rd = (dirs @ M[:3, :3].T).reshape(-1, 3)
        ro = M[:3, 3].expand(rd.shape)
        if ndc:
            t = -(near + ro[:, 2]) / rd[:, 2]
            ro = ro + t[:, None] * rd
            o0 = -1.0 / (W / (2.0 * f)) * ro[:, 0] / ro[:, 2]
            o1 = -1.0 / (H / (2.0 * f)) * ro[:, 1] / ro[:, 2]
            o2 = 1.0 + 2.0 * near / ro[:, 2]
            d0 = -1.0 / (W / (2.0 * f)) * (rd[:, 0] / rd[:, 2] - ro[:, 0] / ro[:, 2])
            d1 = -1.0 / (H / (2.0 * f)) * (rd[:, 1] / rd[:, 2] - ro[:, 1] / ro[:, 2])
            d2 = -2.0 * near / ro[:, 2]
            ro, rd = torch.stack([o0, o1, o2], -1), torch.stack([d0, d1, d2], -1)
        out.append(torch.cat([ro, rd], 1))
    return torch.cat(out)


def _poses(T, seed):
    gen = torch.Generator().manual_seed(seed)
    poses = torch.zeros(T, 9)
    poses[:, 0] = 1
    poses[:, 4] = 1
    return poses + 0.02 * torch.randn(T, 9, generator=gen)


@pytest.mark.parametrize("ndc", [True, False])
def test_camera_rays_match_float64_reference(ndc):
    import rodynrf
    B, H, W = 3, 37, 53
    c2w = rodynrf.pose_to_mtx(_poses(B, 4))
    c2w[:, :, 3] += torch.tensor([[0.1, -0.2, 0.05], [-0.3, 0.1, 0.2], [0.0, 0.0, -0.1]])
    focal = torch.tensor([40.0, 47.5, 61.25])
    rays = rodynrf.camera_rays(c2w.cuda(), focal.cuda(), H, W, ndc=ndc, near=1.0)
    assert rays.shape == (B * H * W, 6)
    ref = _camera_rays_f64(c2w, focal, H, W, ndc)
    assert_close(rays, ref, "camera rays", rtol=1e-5)
    part = rodynrf.camera_rays(c2w.cuda(), focal.cuda(), H, W, ndc=ndc, first=H * W - 7, n=100)
    assert torch.equal(part, rays[H * W - 7:H * W + 93])
    one = rodynrf.camera_rays(c2w[1].cuda(), float(focal[1]), H, W, ndc=ndc)
    assert torch.equal(one, rays[H * W:2 * H * W])
    with pytest.raises(rodynrf.RdrfError):
        rodynrf.camera_rays(c2w.cuda(), focal.cuda(), H, W, first=B * H * W - 3, n=4)


def test_render_view_matches_render_frame_and_the_oracle_pipeline():
    """render_view with c2w = pose_to_mtx(poses9[f]) renders the training camera of frame f: the same maps as
    render_frame(frame=f, maps=True) and the oracle's generate_rays -> sampleXYZ -> fields -> raw2outputs (rtol 2e-4:
    the two ray generators orthonormalise the pose in different orders)"""
    import rodynrf
    from _gpu_util import fields_from_case, oracle_cfg, oracle_sd
    from oracle import rodynrf_oracle as O
    g, st, dy, _ = fields_from_case("ndc_relu")
    T, H, W, frame, S = 5, 9, 16, 3, 21
    poses = _poses(T, 2)
    focal = max(H, W) / 2.0 * 1.7320508
    tv = 2.0 * frame / (T - 1) - 1.0
    fr = rodynrf.render_frame(st, dy, poses.cuda(), focal, frame, H, W, N_samples=S, maps=True)
    rgb, depth = rodynrf.render_frame(st, dy, poses.cuda(), focal, frame, H, W, N_samples=S)
    assert torch.equal(fr.rgb, rgb) and torch.equal(fr.depth, depth)
    _maps_equal(fr, rodynrf.render_frame(st, dy, poses.cuda(), focal, frame, H, W, N_samples=S, maps=True, chunk=50))
    vw = rodynrf.render_view(st, dy, rodynrf.pose_to_mtx(poses[frame]), focal, H, W, tv, N_samples=S)
    ids = torch.arange(H * W) + frame * H * W
    rays = O.generate_rays(ids, poses, focal, H, W, ndc=True, near=1.0)
    ts = torch.full((H * W,), tv)
    xyz, z, valid = O.sampleXYZ(rays, st.aabb.cpu(), [float(v) for v in st.near_far], S, "ndc", None)
    r_s = O.field_forward(oracle_sd(st), oracle_cfg(st), rays, ts, xyz, z, valid, "ndc", dynamic=False)
    r_d = O.field_forward(oracle_sd(dy), oracle_cfg(dy), rays, ts, xyz, z, valid, "ndc", dynamic=True)
    outs = O.raw2outputs(r_s[6], r_s[7], r_d[6], r_d[7], r_d[9], r_d[2], r_d[8], rays, False, "ndc")
    for n, i in OUT_INDEX.items():
        ref = outs[i].clamp(0, 1) if n in ("rgb", "rgb_s", "rgb_d", "blending") else outs[i]
        shape = (H, W, 3) if n.startswith("rgb") else (H, W)
        assert getattr(fr, n).shape == shape and getattr(vw, n).shape == shape, n
        assert_close(getattr(fr, n).reshape(ref.shape), ref, f"frame {n}", rtol=2e-4)
        assert_close(getattr(vw, n).reshape(ref.shape), ref, f"view {n}", rtol=2e-4)
        assert_close(getattr(vw, n), getattr(fr, n), f"view vs frame {n}", rtol=2e-4)


@pytest.mark.parametrize("change_time", ["change", 0.25])
def test_render_path_frames_equal_single_views(change_time):
    import rodynrf
    from _gpu_util import fields_from_case
    g, st, dy, _ = fields_from_case("contract_relu_te")
    n, H, W, S = 4, 11, 13, 19
    c2ws = rodynrf.pose_to_mtx(_poses(n, 8))
    focal = [14.0, 15.0, 16.5, 18.0]
    frames = list(rodynrf.render_path(st, dy, c2ws, focal, H, W, change_time, N_samples=S, ray_type="contract"))
    assert len(frames) == n
    for idx, fr in enumerate(frames):
        t = (round(idx / (n - 1) * (n - 1)) / (n - 1) * 2.0 - 1.0) if change_time == "change" else change_time
        assert rodynrf.path_time(change_time, idx, n) == t
        one = rodynrf.render_view(st, dy, c2ws[idx], focal[idx], H, W, t, N_samples=S, ray_type="contract")
        _maps_equal(fr, one)
    assert not torch.equal(frames[0].rgb_d, frames[-1].rgb_d)


# ---- SSIM -------------------------------------------------------------------------------------------------------
def _ssim_f64(img0, img1, max_val=1.0):
    """utils.py:98-151 rgb_ssim in float64 numpy (scipy.signal.convolve2d 'valid' = a correlation with the flipped
    filter); the pixels are upcast to float64 before the products"""
    img0, img1 = np.asarray(img0, np.float64), np.asarray(img1, np.float64)
    size, sigma, k1, k2 = 11, 1.5, 0.01, 0.03
    hw = size // 2
    shift = (2 * hw - size + 1) / 2
    filt = np.exp(-0.5 * ((np.arange(size) - hw + shift) / sigma) ** 2)
    filt /= np.sum(filt)
    fl = filt[::-1]

    def conv(z, axis):
        n = z.shape[axis] - size + 1
        sl = lambda k: (slice(k, k + n), slice(None)) if axis == 0 else (slice(None), slice(k, k + n))
        return sum(fl[k] * z[sl(k)] for k in range(size))

    filt_fn = lambda z: np.stack([conv(conv(z[..., i], 0), 1) for i in range(z.shape[-1])], -1)
    mu0, mu1 = filt_fn(img0), filt_fn(img1)
    mu00, mu11, mu01 = mu0 * mu0, mu1 * mu1, mu0 * mu1
    s00 = np.maximum(0.0, filt_fn(img0 ** 2) - mu00)
    s11 = np.maximum(0.0, filt_fn(img1 ** 2) - mu11)
    s01 = filt_fn(img0 * img1) - mu01
    s01 = np.sign(s01) * np.minimum(np.sqrt(s00 * s11), np.abs(s01))
    c1, c2 = (k1 * max_val) ** 2, (k2 * max_val) ** 2
    m = (2 * mu01 + c1) * (2 * s01 + c2) / ((mu00 + mu11 + c1) * (s00 + s11 + c2))
    return m, float(np.mean(m))


def _pair(H, W, seed, kind):
    gen = torch.Generator().manual_seed(seed)
    a = torch.rand(H, W, 3, generator=gen)
    if kind == "random":
        b = torch.rand(H, W, 3, generator=gen)
    elif kind == "noisy":
        b = (a + 0.05 * torch.randn(H, W, 3, generator=gen)).clamp(0, 1)
    else:   # flat regions: constant blocks beside texture
        a[: H // 2] = 0.25
        b = a.clone()
        b[: H // 2] = 0.75
        b[H // 2:, : W // 3] = 0.5
    return a, b


@pytest.mark.parametrize("H,W,kind", [(11, 11, "random"), (64, 80, "random"), (64, 80, "flat"), (135, 240, "noisy"),
                                      (135, 240, "random"), (1080, 1920, "noisy")])
def test_ssim_matches_float64_reference(H, W, kind):
    import rodynrf
    a, b = _pair(H, W, H + W, kind)
    ref_map, ref = _ssim_f64(a.numpy(), b.numpy())
    got = rodynrf.ssim(a.cuda(), b.cuda())
    assert got.dim() == 0 and got.dtype == torch.float64
    assert abs(float(got) - ref) <= 1e-10 * abs(ref), (float(got), ref)
    m = rodynrf.ssim(a.cuda(), b.cuda(), return_map=True)
    assert m.shape == (H - 10, W - 10, 3) and m.dtype == torch.float32
    assert float((m.cpu().double() - torch.from_numpy(ref_map)).abs().max()) <= 1e-7
    assert torch.equal(rodynrf.ssim(a.cuda(), b.cuda()), got)   # fixed-order reduction: same bits every call


def test_ssim_identical_pair_max_val_and_errors():
    import rodynrf
    a, b = _pair(135, 240, 3, "noisy")
    assert abs(float(rodynrf.ssim(a.cuda(), a.cuda())) - 1.0) <= 1e-12
    _, ref = _ssim_f64(255.0 * a.numpy(), 255.0 * b.numpy(), max_val=255.0)
    got = float(rodynrf.ssim(255.0 * a.cuda(), 255.0 * b.cuda(), max_val=255.0))
    assert abs(got - ref) <= 1e-10 * abs(ref)
    with pytest.raises(rodynrf.RdrfError):
        rodynrf.ssim(a, b)
    with pytest.raises(rodynrf.RdrfError):
        rodynrf.ssim(a.cuda(), b[:, :-1].cuda())
    with pytest.raises(rodynrf.RdrfError):
        rodynrf.ssim(a[:10].cuda(), b[:10].cuda())
    with pytest.raises(rodynrf.RdrfError):
        rodynrf.ssim(a[:, :10].cuda(), b[:, :10].cuda())
