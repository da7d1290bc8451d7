"""GPU parity of the per-point building blocks the reference's forward() is made of --
compute_densityfeature / compute_appfeature / compute_blendingfeature / warp_coordinate of both fields
(models/tensoRF.py:118-196, 521-811) -- through rdrf_*_features_fwd/bwd, plus the remaining wrappers of
the call surface (OctreeRender_trilinear_fast, sample_ray_ndc / sample_ray_contracted).

Values: the reference's own fn.* vectors of all five fixtures, which include the out-of-range points
(|x| > 1, e.g. (2.5, -3.0, 0.1)) that pin grid_sample's zero padding.  Gradients: the reference's autograd
(tests/golden/fn_grads.npz) and the oracle's autograd on seeded weights at a ragged batch size."""
import os

import numpy as np
import pytest
import torch

from _util import CASES, GOLDEN, assert_close, pkg

pytestmark = pytest.mark.gpu


def _fn_outputs(st, dy, xn, t):
    xu = dy.unnormalize_coord(xn)
    return {"s_density": st.compute_densityfeature(xn, t, None), "s_app": st.compute_appfeature(xn, t, None),
            "d_density": dy.compute_densityfeature(xn, t, None),
            "d_blending": dy.compute_blendingfeature(xn, t, None),
            "d_app": dy.compute_appfeature(xn, t, None), "d_warp": dy.warp_coordinate(xu, t)}, xu


@pytest.mark.parametrize("case", CASES)
def test_golden_function_vectors(case):
    from _gpu_util import fields_from_case
    g, st, dy, _ = fields_from_case(case)
    xn = torch.from_numpy(g["fn.xn"]).cuda()
    t = torch.from_numpy(g["fn.t"]).cuda()
    assert float(np.abs(g["fn.xn"]).max()) > 2.0      # the out-of-range points are in the batch
    with torch.no_grad():
        outs, _ = _fn_outputs(st, dy, xn, t)
    for k, v in outs.items():
        assert v.shape == g["fn." + k].shape, k
        assert_close(v, g["fn." + k], "fn." + k)
    assert st.warp_coordinate(xn, t) is None            # the static field has no warp (tensoRF.py: returns None)


def test_golden_function_gradients():
    """d(sum_k <fn_k, r_k>) wrt every parameter of both fields and wrt the coordinates vs the
    reference's autograd."""
    from _gpu_util import fields_from_case
    g, st, dy, _ = fields_from_case("ndc_relu")
    fg = np.load(os.path.join(GOLDEN, "fn_grads.npz"))
    xn = torch.from_numpy(g["fn.xn"]).cuda().requires_grad_(True)
    t = torch.from_numpy(g["fn.t"]).cuda()
    xu = dy.unnormalize_coord(torch.from_numpy(g["fn.xn"]).cuda()).requires_grad_(True)
    outs = {"s_density": st.compute_densityfeature(xn, t, None), "s_app": st.compute_appfeature(xn, t, None),
            "d_density": dy.compute_densityfeature(xn, t, None),
            "d_blending": dy.compute_blendingfeature(xn, t, None),
            "d_app": dy.compute_appfeature(xn, t, None), "d_warp": dy.warp_coordinate(xu, t)}
    L = 0.0
    for k, v in outs.items():
        L = L + (v * torch.from_numpy(fg["lw." + k]).cuda()).sum()
    assert_close(L, fg["loss"], "loss", rtol=1e-4)
    L.backward()
    bad = []
    for mod, pre in ((st, "gs."), (dy, "gd.")):
        for k, p in mod.named_parameters():
            ref = fg[pre + k]
            if ref.shape == ():
                assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
                continue
            try:
                assert_close(p.grad, ref, pre + k, rtol=2e-4)
            except AssertionError as e:
                bad.append(str(e))
    for name, ten in (("g.xn", xn), ("g.xu", xu)):
        try:
            assert_close(ten.grad, fg[name], name, rtol=2e-4)
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("M", [1, 33, 1000])
def test_function_gradients_vs_oracle(M):
    """seeded weights on a 40x44x26 grid, ragged batch sizes (M = 1, 33, 1000: not multiples of the
    32-point tile), a few points outside [-1,1]^3; every function separately (so a gradient that leaks
    between the entry points cannot cancel), against the oracle's autograd."""
    import rodynrf
    from _gpu_util import COMMON, oracle_cfg, oracle_sd
    from oracle import rodynrf_oracle as O
    torch.manual_seed(100 + M)
    grid = [40, 44, 26]
    aabb = torch.tensor([[-1.5, -1.67, -1.0], [1.5, 1.67, 1.0]])
    kw = dict(COMMON, near_far=[0.0, 1.0], density_shift=-10.0, fea2denseAct="relu")
    st = rodynrf.TensorVMSplit(aabb, grid, 12, "cuda", shadingMode="MLP_Fea", fea_pe=2, **kw)
    dy = rodynrf.TensorVMSplit_TimeEmbedding(aabb, grid, 12, "cuda", shadingMode="MLP_Fea_late_view",
                                             fea_pe=0, **kw)
    gen = torch.Generator().manual_seed(M)
    xn0 = torch.empty(M, 3).uniform_(-1.1, 1.1, generator=gen)
    t0 = torch.randint(0, 12, (M,), generator=gen).float() * 2 / 11 - 1
    sd_s, sd_d = oracle_sd(st), oracle_sd(dy)
    for sd in (sd_s, sd_d):
        for v in sd.values():
            v.requires_grad_(True)
    A = aabb
    fns = {
        "s_density": (lambda x, xu: O.static_density_feature(sd_s, x), lambda x, xu, t: st.compute_densityfeature(x, t, None)),
        "s_app": (lambda x, xu: O.static_app_feature(sd_s, x), lambda x, xu, t: st.compute_appfeature(x, t, None)),
        "d_density": (lambda x, xu: O.dyn_density_feature(sd_d, A, x, t0), lambda x, xu, t: dy.compute_densityfeature(x, t, None)),
        "d_blending": (lambda x, xu: O.dyn_blending_feature(sd_d, A, x, t0), lambda x, xu, t: dy.compute_blendingfeature(x, t, None)),
        "d_app": (lambda x, xu: O.dyn_app_feature(sd_d, A, x, t0), lambda x, xu, t: dy.compute_appfeature(x, t, None)),
        "d_warp": (lambda x, xu: O.warp_coordinate(sd_d, A, xu, t0), lambda x, xu, t: dy.warp_coordinate(xu, t)),
    }
    ks, kd = list(sd_s.keys()), list(sd_d.keys())
    bad = []
    for name, (f_ref, f_gpu) in fns.items():
        xr = xn0.clone().requires_grad_(True)
        xur = O.unnormalize_coord(xn0, A).clone().requires_grad_(True)
        out_r = f_ref(xr, xur)
        r = torch.randn(out_r.shape, generator=gen)
        gref = torch.autograd.grad((out_r * r).sum(), [sd_s[k] for k in ks] + [sd_d[k] for k in kd] + [xr, xur],
                                   allow_unused=True)
        for m in (st, dy):
            for p in m.parameters():
                p.grad = None
        xg = xn0.clone().cuda().requires_grad_(True)
        xug = O.unnormalize_coord(xn0, A).clone().cuda().requires_grad_(True)
        out_g = f_gpu(xg, xug, t0.cuda())
        assert_close(out_g, out_r, name)
        (out_g * r.cuda()).sum().backward()
        own = {"gs." + k: v.grad for k, v in st.named_parameters()}
        own.update({"gd." + k: v.grad for k, v in dy.named_parameters()})
        own["x"], own["xu"] = xg.grad, xug.grad
        for key, gr in zip(["gs." + k for k in ks] + ["gd." + k for k in kd] + ["x", "xu"], gref):
            mine = own[key]
            if gr is None or float(gr.abs().max()) == 0.0:
                assert mine is None or float(mine.abs().max()) == 0.0, f"{name}: {key} should get no gradient"
                continue
            assert mine is not None, f"{name}: no gradient for {key}"
            try:
                assert_close(mine, gr, f"{name}: {key}", rtol=2e-4)
            except AssertionError as e:
                bad.append(str(e))
    assert not bad, "\n".join(bad)


def test_features_fused_grad_and_no_grad_paths():
    """fused_grad accumulates the compute_* gradients straight into the flat buffer; under no_grad
    nothing is saved; a second backward raises instead of crashing."""
    from _gpu_util import fields_from_case
    L = pkg()
    g, st, dy, _ = fields_from_case("ndc_relu")
    xn = torch.from_numpy(g["fn.xn"]).cuda()
    t = torch.from_numpy(g["fn.t"]).cuda()
    loss = lambda: (dy.compute_densityfeature(xn, t, None).sum() + dy.compute_appfeature(xn, t, None).sum()
                    + st.compute_appfeature(xn, t, None).pow(2).sum())
    loss().backward()
    ref = {id(p): p.grad.clone() for m in (st, dy) for p in m.parameters() if p.grad is not None}
    for m in (st, dy):
        for p in m.parameters():
            p.grad = None
        m.fused_grad = True
        m.zero_grad_fused()
    loss().backward()
    n = 0
    for m in (st, dy):
        for p in m._param_list():
            if id(p) in ref:
                assert_close(p.grad, ref[id(p)], "fused", rtol=2e-5)
                n += 1
    assert n > 20
    out = dy.compute_blendingfeature(xn, t, None)
    out.sum().backward(retain_graph=True)
    with pytest.raises(L.RdrfError):
        out.sum().backward()


def test_octree_render_trilinear_fast_matches_direct_calls():
    """renderer.py:24-144: the chunk loop returns the 11-tuple (None, None, blending, pts_ref, weights,
    delta_xyz, None, rgb, sigma, z_vals, dists) concatenated over chunks; for the static field the
    None entries stay None (the reference crashes on them)."""
    import rodynrf
    from _gpu_util import fields_from_case
    g, st, dy, _ = fields_from_case("ndc_relu")
    dev = "cuda"
    rays = torch.from_numpy(g["rays"]).to(dev)
    ts = torch.from_numpy(g["ts"]).to(dev)
    xyz = torch.from_numpy(g["xyz"]).to(dev)
    z = torch.from_numpy(g["z"]).to(dev)
    valid = torch.from_numpy(g["valid"]).to(dev)
    S = z.shape[1]
    with torch.no_grad():
        full = dy(rays, ts, None, xyz, z, valid, is_train=False, ray_type="ndc", N_samples=S)
        out = rodynrf.OctreeRender_trilinear_fast(rays, ts, None, dy, xyz, z, valid, chunk=7, N_samples=S,
                                                  ray_type="ndc", device=dev)
        assert len(out) == 11 and out[0] is None and out[1] is None and out[6] is None
        assert torch.equal(out[2], full[2]) and torch.equal(out[3], full[3]) and torch.equal(out[4], full[4])
        assert_close(out[5], g["fd.xyz_prime"] - g["xyz"], "delta_xyz", rtol=1e-4, atol=1e-6)
        assert torch.equal(out[7], full[6]) and torch.equal(out[8], full[7])
        assert torch.equal(out[9], full[8]) and torch.equal(out[10], full[9])
        assert_close(out[7], g["fd.rgb"], "rgb", mask=(np.abs(g["fd.weight"] - 1e-4) > 1e-6)[..., None].repeat(3, -1))
        so = rodynrf.OctreeRender_trilinear_fast(rays.cpu(), ts.cpu(), None, st, xyz.cpu(), z.cpu(), valid.cpu(),
                                                 chunk=5, N_samples=S, ray_type="ndc", device=dev)
        assert so[2] is None and so[5] is None
        assert_close(so[8], g["fs.sigma"], "static sigma")
        assert_close(so[4], g["fs.weight"], "static weight")


@pytest.mark.parametrize("case", ["ndc_relu_long", "contract_relu_te"])
def test_sample_ray_wrappers(case):
    """TensorBase.sample_ray_ndc / sample_ray_contracted (models/tensorBase.py:487-559): (xyz [N,S,3],
    z row [1,S], valid [N,S]) -- bit-exact against the reference fixture."""
    from _gpu_util import fields_from_case
    g, st, dy, _ = fields_from_case(case)
    rt = str(g["meta.ray_type"])
    rays = torch.from_numpy(g["rays"]).cuda()
    S = g["z"].shape[1]
    # the wrappers draw their own jitter; pin them through is_train=False vs the oracle instead
    from oracle import rodynrf_oracle as O
    xyz_r, z_r, valid_r = O.sampleXYZ(rays.cpu(), dy.aabb.cpu(), [float(v) for v in dy.near_far], S, rt, None, None)
    fn = dy.sample_ray_ndc if rt == "ndc" else dy.sample_ray_contracted
    xyz, zrow, valid = fn(rays[:, :3], rays[:, 3:6], is_train=False, N_samples=S)
    assert zrow.shape == (1, S) and xyz.shape == (rays.shape[0], S, 3)
    assert torch.equal(zrow.cpu(), z_r[:1]) and torch.equal(xyz.cpu(), xyz_r) and torch.equal(valid.cpu(), valid_r)


def test_packed_weight_images_follow_the_weights():
    """The packed MLP images are cached per (weights, stream): an optimiser-style in-place update, a `.data` edit
    followed by invalidate_packed(), and a FlatAdam step must all be seen by the next call; results equal the
    uncached path bit for bit."""
    import rodynrf
    from _gpu_util import COMMON, make_rays
    F = pkg("fields")
    O_ = pkg("optim")
    torch.manual_seed(2)
    aabb = torch.tensor([[-1.5, -1.67, -1.0], [1.5, 1.67, 1.0]])
    kw = dict(COMMON, near_far=[0.0, 1.0], density_shift=-10.0, fea2denseAct="relu")
    st = rodynrf.TensorVMSplit(aabb, [20, 22, 14], 12, "cuda", shadingMode="MLP_Fea", fea_pe=2, **kw)
    dy = rodynrf.TensorVMSplit_TimeEmbedding(aabb, [20, 22, 14], 12, "cuda", shadingMode="MLP_Fea_late_view", fea_pe=0, **kw)
    rays, ts = make_rays(64, 3)
    rays, ts = rays.cuda(), ts.cuda()

    def run():
        with torch.no_grad():
            xyz, z, valid = rodynrf.sampleXYZ(dy, rays, 16, ray_type="ndc", is_train=False)
            a = st(rays, ts, None, xyz, z, valid, is_train=False, ray_type="ndc")[6]
            b = dy(rays, ts, None, xyz, z, valid, is_train=False, ray_type="ndc")[6]
            c = rodynrf.render_rays(st, dy, rays, ts, N_samples=16)[0]
        return a.clone(), b.clone(), c.clone()

    def uncached():
        F.PACK_CACHE = False
        try:
            return run()
        finally:
            F.PACK_CACHE = True

    assert F.PACK_CACHE
    base = run()
    assert all(torch.equal(x, y) for x, y in zip(base, uncached()))
    assert all(torch.equal(x, y) for x, y in zip(base, run()))          # cache hit: identical
    with torch.no_grad():                                                # what torch.optim does
        st.renderModule.mlp[2].weight.mul_(1.5)
        dy.renderModule.mlp[0].bias.add_(0.3)
    upd = run()
    assert not torch.equal(upd[0], base[0]) and not torch.equal(upd[1], base[1]) and not torch.equal(upd[2], base[2])
    assert all(torch.equal(x, y) for x, y in zip(upd, uncached()))
    dy.renderModule.mlp[2].weight.data.mul_(0.5)                         # invisible to the version counter ...
    dy.invalidate_packed()                                               # ... so the caller says so
    upd2 = run()
    assert not torch.equal(upd2[1], upd[1])
    assert all(torch.equal(x, y) for x, y in zip(upd2, uncached()))
    opt = O_.FlatAdam([st, dy], 0.02, 1e-3)                              # raw-pointer Adam: bumps the epoch itself
    loss = st(rays, ts, None, *rodynrf.sampleXYZ(dy, rays, 16, ray_type="ndc", is_train=False), is_train=True,
              ray_type="ndc")[6].sum()
    opt.zero_grad()
    loss.backward()
    opt.step()
    upd3 = run()
    assert not torch.equal(upd3[0], upd2[0])
    assert all(torch.equal(x, y) for x, y in zip(upd3, uncached()))


def test_reference_written_checkpoint_evaluates_like_the_reference():
    """tests/golden/reference_ckpt_*.th (written by the reference's TensorBase.save) loaded on the GPU through the reload
    recipe of train.py:433-447: compute_densityfeature / compute_appfeature at the probe points equal what the
    REFERENCE's own reload of the same file computed (reference_ckpt_probe.npz)."""
    import os
    import numpy as np
    import rodynrf
    from _util import GOLDEN
    probe = np.load(os.path.join(GOLDEN, "reference_ckpt_probe.npz"))
    xn, t = torch.from_numpy(probe["xn"]).cuda(), torch.from_numpy(probe["t"]).cuda()
    for tag, cls in (("static", rodynrf.TensorVMSplit), ("dynamic", rodynrf.TensorVMSplit_TimeEmbedding)):
        ckpt = torch.load(os.path.join(GOLDEN, f"reference_ckpt_{tag}.th"), map_location="cpu", weights_only=False)
        kwargs = dict(ckpt["kwargs"])
        kwargs.pop("se3_poses")
        kwargs.pop("focal_ratio_refine")
        kwargs.update({"device": "cuda:0"})
        m = cls(**kwargs)
        m.load(ckpt)
        with torch.no_grad():
            # (max-norm, like test_golden_function_vectors: the features are cancelling sums of 72 / 216 products)
            assert_close(m.compute_densityfeature(xn, t, None), probe[tag + ".density"], tag + ".density")
            assert_close(m.compute_appfeature(xn, t, None), probe[tag + ".app"], tag + ".app")
