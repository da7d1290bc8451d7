"""GPU parity of the WORLD-space ray path (ray_type "world": every ray_type but "ndc" / "contract"): the sampler
(rdrf_sample_world / _bwd, TensorBase.sample_ray), the fields' forward and raw2outputs on its samples, their gradients, and
the no-grad render family (rdrf_render_world_fwd) against the reference's own outputs (tests/golden/world*.npz, written by
tests/golden/make_golden_world.py) and against a float64 restatement of the sampler."""
import functools
import os

import numpy as np
import pytest
import torch

from _util import GOLDEN, assert_close, pkg

pytestmark = pytest.mark.gpu

NAMES = ["_0", "_1", "blending", "pts_ref", "weight", "xyz_prime", "rgb", "sigma", "z", "dists"]
ONAMES = ["rgb_map_full", "depth_map_full", "acc_map_full", "weights_full", "rgb_map_s", "depth_map_s", "acc_map_s",
          "weights_s", "rgb_map_d", "depth_map_d", "acc_map_d", "weights_d", "dynamicness_map"]
DEV = "cuda"


@functools.lru_cache(maxsize=None)
def fixture():
    g = dict(np.load(os.path.join(GOLDEN, "world.npz")))
    w = np.load(os.path.join(GOLDEN, "world_weights.npz"))
    sd_s = {k[2:]: torch.from_numpy(w[k]) for k in w.files if k.startswith("s.")}
    sd_d = {k[2:]: torch.from_numpy(w[k]) for k in w.files if k.startswith("d.")}
    return g, sd_s, sd_d


@functools.lru_cache(maxsize=None)
def fields(tag):
    """the two HIP-backed fields of configuration `tag` ("a": softplus, "b": relu) on the fixture's weights"""
    import rodynrf
    from _gpu_util import COMMON
    g, sd_s, sd_d = fixture()
    kw = dict(COMMON, near_far=[float(v) for v in g["meta.near_far"]], density_shift=float(g[tag + ".density_shift"]),
              fea2denseAct=str(g[tag + ".act"]), step_ratio=float(g["meta.step_ratio"]))
    aabb, grid = torch.from_numpy(g["aabb"]), [int(v) for v in g["meta.grid"]]
    st = rodynrf.TensorVMSplit(aabb, grid, 12, DEV, shadingMode=str(g["meta.static_head"]), fea_pe=2, **kw)
    dy = rodynrf.TensorVMSplit_TimeEmbedding(aabb, grid, 12, DEV, shadingMode="MLP_Fea_late_view", fea_pe=0, **kw)
    st.load_state_dict(sd_s)
    dy.load_state_dict(sd_d)
    assert np.float32(dy._step_host) == g["meta.stepSize"], "stepSize differs from the reference's"
    return st, dy


def dev(a):
    return torch.from_numpy(np.asarray(a)).to(DEV)


def sample(tag_or_dy, rays, S, train):
    import rodynrf
    g = fixture()[0]
    dy = fields(tag_or_dy)[1] if isinstance(tag_or_dy, str) else tag_or_dy
    return rodynrf.sampleXYZ(dy, rays, S, ray_type="world", is_train=train, jitter=dev(g["u"]) if train else None)


@pytest.mark.parametrize("S", [33, 70])
@pytest.mark.parametrize("mode", ["eval", "train"])
def test_sampler_bits(S, mode):
    """xyz, z_vals (per ray, [N,S]) and the valid mask are the reference's sample_ray bit for bit, through sampleXYZ and
    through TensorBase.sample_ray of either field"""
    g = fixture()[0]
    st, dy = fields("a")
    rays = dev(g["rays"])
    xyz, z, valid = sample("a", rays, S, mode == "train")
    pre = f"{mode}{S}."
    assert z.shape == (rays.shape[0], S)
    assert np.array_equal(z.cpu().numpy(), g[pre + "z"]), "z_vals"
    assert np.array_equal(xyz.cpu().numpy(), g[pre + "xyz"]), "xyz"
    assert np.array_equal(valid.cpu().numpy(), g[pre + "valid"]), "valid"
    if mode == "eval":
        for f in (st, dy):
            x2, z2, v2 = f.sample_ray(rays[:, :3], rays[:, 3:], is_train=False, N_samples=S)
            assert torch.equal(x2, xyz) and torch.equal(z2, z) and torch.equal(v2, valid)
    else:   # a drawn jitter: one value per ray, in [0, 1)
        x3, z3, _ = dy.sample_ray(rays[:, :3], rays[:, 3:], is_train=True, N_samples=S)
        uu = (z3 - dev(g[f"eval{S}.z"])) / dy._step_host
        assert float(uu.min()) > -1e-4 and float(uu.max()) < 1 + 1e-4 and float((uu.max(1)[0] - uu.min(1)[0]).max()) < 1e-3
        assert float(uu[:, 0].std()) > 0.1


def _chain(tag, rays, white):
    import rodynrf
    g = fixture()[0]
    st, dy = fields(tag)
    S, train = int(g[tag + ".S"]), bool(g[tag + ".train"])
    ts = dev(g["ts"])
    xyz, z, valid = sample(tag, rays, S, train)
    o_s = st(rays, ts, None, xyz, z, valid, is_train=True, ray_type="world", N_samples=S)
    o_d = dy(rays, ts, None, xyz, z, valid, is_train=True, ray_type="world", N_samples=S)
    outs = rodynrf.raw2outputs(o_s[6], o_s[7], o_d[6], o_d[7], o_d[9], o_d[2], o_d[8], rays, is_train=white,
                               ray_type="world", add_white_bg=white)
    return (xyz, z, valid), o_s, o_d, outs


@pytest.mark.parametrize("tag", ["a", "b"])
def test_forward_and_composite(tag):
    """the 10-tuples of both fields' forward(..., ray_type="world") and the 13 outputs of raw2outputs(..., ray_type="world")
    (eval, and train with the white background) against the reference: 1e-4 relative to each tensor's max"""
    g = fixture()[0]
    with torch.no_grad():
        rays = dev(g["rays"])
        (xyz, z, valid), o_s, o_d, c_eval = _chain(tag, rays, False)
        c1 = _chain(tag, rays, True)[3]
    for pre, o in (("fs.", o_s), ("fd.", o_d)):
        assert torch.equal(o[3], xyz) and torch.equal(o[8], z)
        for k, v in zip(NAMES, o):
            key = f"{tag}.{pre}{k}"
            if key in g:
                assert_close(v, g[key], key)
            else:
                assert v is None or k in ("pts_ref", "z"), key
    for k, a, c in zip(ONAMES, c_eval, c1):
        assert_close(a, g[f"{tag}.ce.{k}"], f"{tag}.ce.{k}")
        assert_close(c, g[f"{tag}.c1.{k}"], f"{tag}.c1.{k}")
    # rays that miss the box: every sample invalid, nothing accumulated, no far-plane depth, no background in eval mode
    miss = dev(g["kind"] == 8)
    assert int(miss.sum()) >= 3 and not bool(valid[miss].any())
    for i in (0, 1, 2, 4, 5, 6, 8, 9, 10):
        assert float(c_eval[i][miss].abs().max()) == 0.0, ONAMES[i]


def test_gradients():
    """one scalar loss over sampleXYZ -> both fields -> raw2outputs: d loss / d parameter for every parameter of both fields
    and d loss / d rays (through xyz, through z_vals, and through both into t_min) against the reference's autograd"""
    g = fixture()[0]
    gr = np.load(os.path.join(GOLDEN, "world_grads.npz"))
    st, dy = fields("a")
    for m in (st, dy):
        m.zero_grad(set_to_none=True)
    rays = dev(g["rays"]).requires_grad_(True)
    _, o_s, o_d, outs = _chain("a", rays, True)
    L = 0.0
    for k, v in zip(ONAMES, outs):
        L = L + (v * dev(g["lw.c1." + k])).sum()
    for k, v in (("blending", o_d[2]), ("weight", o_d[4]), ("xyz_prime", o_d[5]), ("weight_s", o_s[4])):
        L = L + (v * dev(g["lw.f." + k])).sum()
    assert_close(L, g["loss"], "loss", rtol=2e-4)
    L.backward()
    bad = []
    for mod, pre in ((st, "gs."), (dy, "gd.")):
        for k, p in mod.named_parameters():
            ref = gr[pre + k]
            if ref.shape == ():
                assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
                continue
            assert p.grad is not None, f"no grad for {pre}{k}"
            try:
                assert_close(p.grad, ref, pre + k, rtol=1e-4)
            except AssertionError as e:
                bad.append(str(e))
    try:
        assert_close(rays.grad, g["g.rays"], "g.rays", rtol=1e-4)
    except AssertionError as e:
        bad.append(str(e))
    for m in (st, dy):
        m.zero_grad(set_to_none=True)
    assert not bad, "\n".join(bad)


def _sample_f64(rays, lo, hi, near, far, step, u, S):
    """float64 restatement of the world-space march, differentiable by torch's autograd"""
    o, d = rays[:, :3], rays[:, 3:]
    vec = torch.where(d == 0, torch.full_like(d, 1e-6), d)
    t_min = torch.minimum((hi - o) / vec, (lo - o) / vec).amax(-1).clamp(min=near, max=far)
    z = t_min[:, None] + step * (torch.arange(S, dtype=rays.dtype)[None] + u[:, None])
    return o[:, None, :] + d[:, None, :] * z[..., None], z


@pytest.mark.parametrize("S", [33, 70])
def test_sampler_ray_gradient_float64(S):
    """d / d rays of the sampler alone, from g_xyz and from g_z, against float64 autograd of the restatement above.  Second
    loss: g_xyz is zero on each ray's selected axis, so that axis' two entries of the ray gradient hold the t_min term
    alone -- non-zero where the clamp is inactive, exactly zero where it holds t_min at near / far or the ray's component
    is 0 behind the `where`."""
    g = fixture()[0]
    dy = fields("a")[1]
    N = g["rays"].shape[0]
    gen = torch.Generator().manual_seed(S)
    w, wz = torch.randn(N, S, 3, generator=gen), torch.randn(N, S, generator=gen)
    lo, hi = (torch.from_numpy(g["aabb"][i]).double() for i in (0, 1))
    near, far = (float(v) for v in g["meta.near_far"])
    r64 = torch.from_numpy(g["rays"]).double()
    vec = torch.where(r64[:, 3:] == 0, torch.full_like(r64[:, 3:], 1e-6), r64[:, 3:])
    m = torch.minimum((hi - r64[:, :3]) / vec, (lo - r64[:, :3]) / vec)
    raw, axis = m.max(-1)
    free = (raw > near) & (raw < far)
    assert 20 < int(free.sum()) < N
    w_off = w.clone()
    w_off[torch.arange(N), :, axis] = 0.0
    for name, wx, wzz in (("xyz + z", w, wz), ("xyz off the selected axis", w_off, None)):
        rr = r64.clone().requires_grad_(True)
        xyz, z = _sample_f64(rr, lo, hi, near, far, float(g["meta.stepSize"]), torch.from_numpy(g["u"]).double(), S)
        Lr = (xyz * wx.double()).sum() + (0.0 if wzz is None else (z * wzz.double()).sum())
        gref, = torch.autograd.grad(Lr, rr)
        rays = dev(g["rays"]).requires_grad_(True)
        gx, gz, _ = sample(dy, rays, S, True)
        assert_close(gx, xyz.detach().float(), "xyz vs float64", rtol=1e-6)
        Lg = (gx * wx.to(DEV)).sum() + (0.0 if wzz is None else (gz * wzz.to(DEV)).sum())
        ggot, = torch.autograd.grad(Lg, rays)
        assert_close(ggot, gref, f"d sampler / d rays ({name}, S={S})", rtol=1e-4)
        if wzz is None:
            rows = torch.arange(N)
            sel = torch.stack([ggot.cpu()[rows, axis], ggot.cpu()[rows, 3 + axis]], -1)
            ref = torch.stack([gref[rows, axis], gref[rows, 3 + axis]], -1)
            assert_close(sel, ref, f"t_min term alone (S={S})", rtol=1e-4)
            assert bool((sel[free][:, 0] != 0).all()) and bool((sel[~free] == 0).all())
            dk = r64[rows, 3 + axis]
            assert bool((sel[free & (dk != 0)][:, 1] != 0).all()) and bool((sel[dk == 0][:, 1] == 0).all())


def test_sampler_gradient_behind_the_zero_direction_where():
    """A direction component that is exactly 0 on the SELECTED axis with the clamp inactive (the origin sits 2e-6 outside the
    slab, so the 1e-6 stand-in gives t_min = 2): t_min still depends on o_k (-1 / 1e-6) but not on d_k -- the reference's
    `where` cuts the graph there.  The fixture's own zero components are never selected; this ray is."""
    g = fixture()[0]
    dy = fields("a")[1]
    S = 33
    lo, hi = (torch.from_numpy(g["aabb"][i]) for i in (0, 1))
    near, far = (float(v) for v in g["meta.near_far"])
    rays32 = torch.tensor([[float(lo[0]) - 2e-6, 0.1, 1.0, 0.0, 0.3, 0.2],
                           [0.3, float(lo[1]) - 2e-6, 1.1, -0.2, 0.0, 0.25]])
    u = torch.tensor([0.25, 0.75])
    gen = torch.Generator().manual_seed(3)
    w = torch.randn(2, S, 3, generator=gen)
    rr = rays32.double().requires_grad_(True)
    xyz, z = _sample_f64(rr, lo.double(), hi.double(), near, far, float(g["meta.stepSize"]), u.double(), S)
    assert bool(((z[:, 0] > near + 0.5) & (z[:, 0] < far - 0.5)).all())
    gref, = torch.autograd.grad((xyz * w.double()).sum(), rr)
    rays = rays32.to(DEV).requires_grad_(True)
    import rodynrf
    gx, gz, _ = rodynrf.sampleXYZ(dy, rays, S, ray_type="world", is_train=True, jitter=u.to(DEV))
    ggot, = torch.autograd.grad((gx * w.to(DEV)).sum(), rays)
    for n, k in ((0, 0), (1, 1)):
        assert abs(float(gref[n, k])) > 1e4     # the -1 / 1e-6 slope
        assert_close(ggot[n], gref[n], f"zero-direction ray {n}", rtol=1e-4)
        # d / d d_k: the direct term sum_j g_k z_j only
        assert_close(ggot[n, 3 + k], (w[n, :, k].double() * z[n].detach()).sum(), f"zero-direction ray {n}: d_k", rtol=1e-4)


def test_render_family_bits():
    """render_rays in its three modes (pair and maps), render_chunks (chunk 32 over the 67 rays) and render_view / render_frame
    (a 9 x 7 image) give the bits of the composed call sampleXYZ -> static forward -> dynamic forward -> raw2outputs"""
    import rodynrf
    g = fixture()[0]
    st, dy = fields("a")
    S = 33
    ts = dev(g["ts"])

    def composed(rays, ts):
        with torch.no_grad():
            xyz, z, valid = rodynrf.sampleXYZ(dy, rays, S, ray_type="world", is_train=False)
            o_s = st(rays, ts, None, xyz, z, valid, ray_type="world", N_samples=S)
            o_d = dy(rays, ts, None, xyz, z, valid, ray_type="world", N_samples=S)
            return rodynrf.raw2outputs(o_s[6], o_s[7], o_d[6], o_d[7], o_d[9], o_d[2], o_d[8], rays, is_train=False,
                                       ray_type="world")

    slots = dict(rgb=0, depth=1, acc=2, rgb_s=4, depth_s=5, acc_s=6, rgb_d=8, depth_d=9, acc_d=10, blending=12)

    def same_maps(m, ref, what):
        for n, i in slots.items():
            got = getattr(m, n)
            assert torch.equal(got.reshape(ref[i].shape), ref[i]), f"{what}: {n}"

    rays = dev(g["rays"])
    ref = composed(rays, ts)
    assert float(ref[2].max()) > 0.1 and torch.isfinite(ref[1]).all()
    for mode in ("auto", "fused", "sequence"):
        rgb, depth = rodynrf.render_rays(st, dy, rays, ts, S, ray_type="world", mode=mode)
        assert torch.equal(rgb, ref[0]) and torch.equal(depth, ref[1]), mode
        same_maps(rodynrf.render_rays(st, dy, rays, ts, S, ray_type="world", mode=mode, maps=True), ref, mode)
    rgb, depth = rodynrf.render_chunks(st, dy, rays, ts, 32, S, ray_type="world")
    assert torch.equal(rgb, ref[0]) and torch.equal(depth, ref[1]), "render_chunks"
    same_maps(rodynrf.render_chunks(st, dy, rays, ts, 32, S, ray_type="world", maps=True), ref, "render_chunks maps")
    rgb, depth = rodynrf.render_chunks(st, dy, rays, ts, 32, S, ray_type="world", streams=0)
    assert torch.equal(rgb, ref[0]) and torch.equal(depth, ref[1]), "render_chunks on one stream"
    # a camera 3 units in front of the box's -z face, looking along +z (camera looks down its own -z: flip y and z)
    H, W, focal = 7, 9, 6.0
    c2w = torch.tensor([[1.0, 0.0, 0.0, 0.2], [0.0, -1.0, 0.0, 0.2], [0.0, 0.0, -1.0, -1.5]])
    vrays = rodynrf.camera_rays(c2w.to(DEV), focal, H, W, ndc=False)
    vts = torch.full((H * W,), 0.25, device=DEV)
    vref = composed(vrays, vts)
    assert float(vref[2].max()) > 0.1
    same_maps(rodynrf.render_view(st, dy, c2w, focal, H, W, 0.25, S, ray_type="world", maps=True), vref, "render_view")
    rgb, depth = rodynrf.render_view(st, dy, c2w, focal, H, W, 0.25, S, ray_type="world", maps=False, chunk=20)
    assert torch.equal(rgb.reshape(-1, 3), vref[0]) and torch.equal(depth.reshape(-1), vref[1]), "render_view in chunks"


def test_refusals():
    """what the reference has no world branch for still raises: motion maps and induced flow; and the render entry points of
    the other two ray types refuse a world-space config instead of sampling it as a contracted one"""
    import ctypes as C
    import rodynrf
    L = pkg()
    F = pkg("fields")
    g = fixture()[0]
    st, dy = fields("a")
    rays, ts = dev(g["rays"]), dev(g["ts"])
    N, S = rays.shape[0], 33
    eye = torch.eye(3, 4)
    with pytest.raises(NotImplementedError):
        rodynrf.render_rays(st, dy, rays, ts, S, ray_type="world", motion=dict(H=1, W=N, focal=10.0, c2w_f=eye, c2w_b=eye))
    with pytest.raises(NotImplementedError):
        rodynrf.render_view(st, dy, eye, 6.0, 7, 9, 0.0, S, ray_type="world", motion=True)
    with pytest.raises(L.RdrfError):
        rodynrf.induce_flow(9, 16, 10.0, torch.zeros(N, 3, 4, device=DEV), torch.zeros(N, S, device=DEV),
                            torch.zeros(N, S, 3, device=DEV), torch.zeros(N, 2, device=DEV), rays, ray_type="world")
    with pytest.raises(L.RdrfError):     # one jitter value per ray
        rodynrf.sampleXYZ(dy, rays, S, ray_type="world", is_train=True, jitter=torch.rand(S, device=DEV))
    ps, pd = st._param_list(), dy._param_list()
    PS, PD = F._static_struct(ps), F._dynamic_struct(pd)
    cs, cd = F._cfg_struct(st, "world"), F._cfg_struct(dy, "world")
    rgb, depth = torch.empty(N, 3, device=DEV), torch.empty(N, device=DEV)
    ws = L.workspace(rays.device, int(L.lib.rdrf_render_workspace_bytes(N, S)))
    rc = L.lib.rdrf_render_fwd(C.byref(PS), C.byref(cs), C.byref(PD), C.byref(cd), L.ptr(rays), L.ptr(ts), N, S, C.c_float(0.5),
                               C.c_float(4.0), L.ptr(rgb), L.ptr(depth), L.ptr(ws), C.c_size_t(ws.numel()), L.stream_of(rays))
    assert rc < 0 and b"rdrf_render_world_fwd" in L.lib.rdrf_last_error()
