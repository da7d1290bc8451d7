"""GPU parity of the factor-space kernels: the flat Adam step vs torch.optim.Adam,
the bilinear VM upsampling vs F.interpolate, density_L1 / blending_L1 vs the reference's own values and
gradients (tests/golden/tv.npz) and vs the dense einsum at the Balloon1 grid, and the uv / view-shift ray
generator vs the oracle."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from _util import GOLDEN, assert_close, pkg

pytestmark = pytest.mark.gpu


def test_adam_step_matches_torch_adam():
    L = pkg()
    g = torch.Generator().manual_seed(0)
    n, split = 4096 + 512, 1024
    p0 = torch.randn(n, generator=g)
    ref_a = torch.nn.Parameter(p0[:split].clone().cuda())
    ref_b = torch.nn.Parameter(p0[split:].clone().cuda())
    opt = torch.optim.Adam([{"params": [ref_a], "lr": 0.02}, {"params": [ref_b], "lr": 1e-3}], betas=(0.9, 0.99))
    p = p0.clone().cuda()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for step in range(1, 8):
        grad = (torch.randn(n, generator=g) * (10.0 ** torch.randint(-4, 2, (n,), generator=g).float())).cuda()
        ref_a.grad, ref_b.grad = grad[:split].clone() * 0.5, grad[split:].clone() * 0.5
        opt.step()
        L.check(L.lib.rdrf_adam_step(L.ptr(p), L.ptr(grad), L.ptr(m), L.ptr(v), C.c_size_t(n), C.c_size_t(split), 0.02,
                                     1e-3, 0.9, 0.99, 1e-8, step, 0.5, L.stream_of(p)), "adam")
        assert_close(p[:split], ref_a, f"step {step} lr0", rtol=2e-6)
        assert_close(p[split:], ref_b, f"step {step} lr1", rtol=2e-6)
    assert L.lib.rdrf_adam_step(L.ptr(p), L.ptr(grad), L.ptr(m), L.ptr(v), C.c_size_t(n - 1), C.c_size_t(split), 0.02, 1e-3,
                                0.9, 0.99, 1e-8, 1, 1.0, L.stream_of(p)) < 0


def test_flat_adam_trains_like_torch_adam_on_the_fields():
    """FlatAdam over the flattened parameters of both fields == torch.optim.Adam over get_optparam_groups (the
    reference's optimiser), three steps on a real loss; parameters stay views of the flat buffer and
    state_dict() keeps the reference's keys / shapes."""
    import rodynrf
    from _gpu_util import fields_from_case
    O = pkg("optim")
    g, st, dy, _ = fields_from_case("ndc_relu")
    g2, st2, dy2, _ = fields_from_case("ndc_relu")
    dev = "cuda"
    rays = torch.from_numpy(g["rays"]).to(dev)
    ts = torch.from_numpy(g["ts"]).to(dev)
    xyz = torch.from_numpy(g["xyz"]).to(dev)
    z = torch.from_numpy(g["z"]).to(dev)
    valid = torch.from_numpy(g["valid"]).to(dev)

    def loss_of(a, b):
        o_s = a(rays, ts, None, xyz, z, valid, ray_type="ndc")
        o_d = b(rays, ts, None, xyz, z, valid, ray_type="ndc")
        outs = rodynrf.raw2outputs(o_s[6], o_s[7], o_d[6], o_d[7], o_d[9], o_d[2], o_d[8], rays, is_train=True,
                                   ray_type="ndc", add_white_bg=False)
        return (outs[0] ** 2).sum() + outs[9].sum() + (outs[4] ** 2).sum() + (o_d[5] ** 2).mean()

    keys = list(st.state_dict().keys())
    opt = O.FlatAdam([st, dy], 0.02, 1e-3, lr_factor=0.9)
    ref = torch.optim.Adam(st2.get_optparam_groups(0.02, 1e-3) + dy2.get_optparam_groups(0.02, 1e-3), betas=(0.9, 0.99))
    assert list(st.state_dict().keys()) == keys
    for it in range(3):
        opt.zero_grad()
        loss_of(st, dy).backward()
        opt.step()
        ref.zero_grad()
        loss_of(st2, dy2).backward()
        ref.step()
        for gr in ref.param_groups:
            gr["lr"] *= 0.9
    flat = st.flatten_params_()
    for (k, a), (_, b) in zip(list(st.state_dict().items()) + list(dy.state_dict().items()),
                              list(st2.state_dict().items()) + list(dy2.state_dict().items())):
        assert a.shape == b.shape
        assert_close(a, b, k, rtol=2e-4)
    p = st._param_list()[0]
    assert flat.data_ptr() <= p.data_ptr() < flat.data_ptr() + flat.numel() * 4 and p.stride(1) == 1


def test_dense_l1_matches_reference_fixture():
    from _gpu_util import fields_from_case
    g, st, dy, _ = fields_from_case("ndc_relu")
    tv = np.load(os.path.join(GOLDEN, "tv.npz"))
    for tag, mod, names in (("s", st, ("density_L1",)), ("d", dy, ("density_L1", "blending_L1"))):
        for nm in names:
            fam = "blending" if nm == "blending_L1" else "density"
            ps = list(getattr(mod, f"{fam}_plane")) + list(getattr(mod, f"{fam}_line"))
            for p in ps:
                p.grad = None
            val = getattr(mod, nm)()
            assert_close(val, tv[f"r.{tag}.{nm}.value"], f"{tag}.{nm}", rtol=1e-5)
            (val * 3.0).backward()
            for i, p in enumerate(ps):
                assert_close(p.grad / 3.0, tv[f"r.{tag}.{nm}.g{i}"], f"{tag}.{nm}.g{i}", rtol=2e-5)


@pytest.mark.parametrize("act", ["relu", "softplus"])
def test_dense_l1_balloon_grid_vs_einsum(act):
    import rodynrf
    from _gpu_util import COMMON
    torch.manual_seed(5)
    aabb = torch.tensor([[-1.5, -1.67, -1.0], [1.5, 1.67, 1.0]])
    kw = dict(COMMON, near_far=[0.0, 1.0], density_shift=-1.0, fea2denseAct=act)
    dy = rodynrf.TensorVMSplit_TimeEmbedding(aabb, [141, 157, 94], 12, "cuda", shadingMode="MLP_Fea_late_view",
                                             fea_pe=0, **kw)
    planes, lines = list(dy.density_plane), list(dy.density_line)
    p0, p1, p2 = (p[0] for p in planes)
    l0, l1, l2 = (l[0, :, :, 0] for l in lines)
    f = torch.einsum("cyx,cz->xyz", p0, l0) + torch.einsum("czx,cy->xyz", p1, l1) + torch.einsum("czy,cx->xyz", p2, l2)
    ref = dy.feature2density(f).abs().mean()
    gref = torch.autograd.grad(ref, planes + lines)
    val = dy.density_L1()
    assert_close(val, ref, "value", rtol=2e-5)
    gown = torch.autograd.grad(val, planes + lines)
    for i, (a, b) in enumerate(zip(gown, gref)):
        assert a.stride() == (planes + lines)[i].stride()
        assert_close(a, b, f"grad {i}", rtol=5e-5)


def test_upsample_kernel_matches_interpolate():
    import rodynrf
    from _gpu_util import COMMON
    torch.manual_seed(6)
    aabb = torch.tensor([[-1.5, -1.67, -1.0], [1.5, 1.67, 1.0]])
    kw = dict(COMMON, near_far=[0.0, 1.0], density_shift=-10.0, fea2denseAct="relu")
    st = rodynrf.TensorVMSplit(aabb, [17, 19, 11], 12, "cuda", shadingMode="MLP_Fea", fea_pe=2, **kw)
    before = {k: v.detach().cpu().contiguous() for k, v in st.state_dict().items() if "_plane" in k or "_line" in k}
    for new in ([33, 37, 22], [141, 157, 94], [20, 18, 13]):   # up, up, then DOWN (interpolate handles both)
        st.upsample_volume_grid(new)
        for k, v in st.state_dict().items():
            if k in before:
                want = torch.nn.functional.interpolate(before[k], size=v.shape[2:], mode="bilinear", align_corners=True)
                assert v.stride(1) == 1
                assert_close(v, want, k, rtol=2e-6)
                before[k] = v.detach().cpu().contiguous()
        assert st.gridSize.tolist() == new


def test_generate_rays_uv_and_view_shift():
    import rodynrf
    from oracle import rodynrf_oracle as O
    gen = torch.Generator().manual_seed(8)
    T, H, W, N = 5, 27, 48, 200
    poses = torch.zeros(T, 9)
    poses[:, 0] = 1
    poses[:, 4] = 1
    poses = poses + 0.05 * torch.randn(T, 9, generator=gen)
    ids = torch.randint(0, T * H * W, (N,), generator=gen)
    ids[:4] = torch.tensor([0, 5, T * H * W - 1, T * H * W - 7])        # first / last frame: the shift clamps
    col, row, _ = O.ids2pixel(W, H, ids)
    uv = torch.stack([col.float() + 0.5, row.float() + 0.5], -1) + 2.0 * torch.randn(N, 2, generator=gen)
    lw = torch.randn(N, 6, generator=gen)
    for ndc in (True, False):
        for shift in (1, -1, 0):
            pr = poses.clone().requires_grad_(True)
            fr = torch.tensor(max(H, W) / 2.0 * 1.7320508, requires_grad=True)
            ref = O.generate_rays(ids, pr, fr, H, W, ndc=ndc, near=1.0, uv=uv, view_shift=shift)
            gp, gf = torch.autograd.grad((ref * lw).sum(), [pr, fr])
            pg = poses.clone().cuda().requires_grad_(True)
            fg = torch.tensor([max(H, W) / 2.0 * 1.7320508], device="cuda", requires_grad=True)   # focal of shape [1]
            rays = rodynrf.generate_rays(ids.cuda(), pg, fg, H, W, ndc=ndc, near=1.0, uv=uv.cuda(), view_shift=shift)
            assert_close(rays, ref, f"rays ndc={ndc} shift={shift}", rtol=2e-5)
            (rays * lw.cuda()).sum().backward()
            assert fg.grad.shape == (1,)
            assert_close(pg.grad, gp, "g_poses", rtol=3e-4)
            assert_close(fg.grad[0], gf, "g_focal", rtol=3e-4)
