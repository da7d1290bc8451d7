"""Deterministic build (RDRF_DETERMINISTIC=1, librodynrf_det.so): every translation unit whose kernels call grad_add holds
its own copy of the slot table g_det (csrc/rdrf_common.hpp), and rdrf_det_bind has to write all of them (RDRF_DET_UNIT,
csrc/rdrf_det.hip).  A unit whose copy was not bound adds with plain fp32 atomics: almost the right numbers, no longer
bit-reproducible, and no parity test notices.

This test does: between a backward and det_fold_() EVERY parameter-gradient addition must sit in the fixed-point shadow,
so the field's flat fp32 gradient buffer is still exactly zero everywhere; the fold then moves the sums over and clears
the shadow.  It runs the launches of every unit that adds parameter gradients -- backward-data kernels (rdrf_bwd.hip), ray
and sorted / tiled scatter (rdrf_scatter.hip), dW products (rdrf_dw.hip) -- through the ray path of both fields, the
sorted scatter mode, feature mode and scene flow, at the shapes of smoke().  No parameter slice is excluded from the
zero assertion: no kernel of these paths writes a parameter gradient other than through grad_add."""
import json

import pytest

from _twin import CHILD, run_twin
from _util import pkg

pytestmark = pytest.mark.gpu


def det_case():
    """what the deterministic library runs (tests/_det_child.py case): one report line per step"""
    import torch
    import rodynrf
    from _gpu_util import COMMON, make_rays
    L = pkg()
    torch.manual_seed(3)
    N, S, M, grid = 48, 40, 100, [24, 26, 16]
    dev = "cuda:0"
    aabb = torch.tensor([[-1.5, -1.67, -1.0], [1.5, 1.67, 1.0]])
    kw = dict(COMMON, near_far=[0.0, 1.0], density_shift=-10.0, fea2denseAct="relu")
    st = rodynrf.TensorVMSplit(aabb, grid, 12, dev, shadingMode="MLP_Fea", fea_pe=2, **kw)
    dy = rodynrf.TensorVMSplit_TimeEmbedding(aabb, grid, 12, dev, shadingMode="MLP_Fea_late_view", fea_pe=0, **kw)
    for f in (st, dy):
        f.fused_grad = True
        f.zero_grad_fused()
    rays, ts = make_rays(N, 1)
    cr, ct = rays.to(dev), ts.to(dev)
    jit = torch.rand(S, generator=torch.Generator().manual_seed(2)).to(dev)
    gx, gz, gv = rodynrf.sampleXYZ(dy, cr, S, ray_type="ndc", is_train=True, jitter=jit)
    gen = torch.Generator().manual_seed(7)
    w_rgb = torch.rand(N, S, 3, generator=gen).to(dev)
    w_ns = [torch.rand(N, S, generator=gen).to(dev) + 0.5 for _ in range(3)]
    xn = (torch.rand(M, 3, generator=gen) * 1.9 - 0.95).to(dev)
    tm = (torch.rand(M, generator=gen) * 2 - 1).to(dev)
    report, bad = [], []

    def slices(field, flat):
        """names of the parameters whose slice of `flat` has a non-zero entry"""
        offs, _, _ = field._flat_layout()
        names = {p.data_ptr(): n for n, p in field.named_parameters()}
        return [names.get(p.data_ptr(), "?") for p, o in zip(field._param_list(), offs) if bool((flat[o:o + p.numel()] != 0).any())]

    def check(step, field):
        torch.cuda.synchronize()
        g, sh = field._gflat, field._det_shadow
        pre = {"step": step, "gflat_nonzero_before_fold": int((g != 0).sum()), "gflat_absmax_before_fold": float(g.abs().max()),
               "gflat_slices_before_fold": slices(field, g), "shadow_nonzero_before_fold": int((sh != 0).sum())}
        field.det_fold_()
        torch.cuda.synchronize()
        pre.update(gflat_nonzero_after_fold=int((g != 0).sum()), shadow_nonzero_after_fold=int((sh != 0).sum()))
        report.append(pre)
        print(json.dumps(pre), flush=True)
        if pre["gflat_nonzero_before_fold"] != 0:
            bad.append(f"{step}: {pre['gflat_nonzero_before_fold']} fp32 gradient entries were written before the fold "
                       f"(max {pre['gflat_absmax_before_fold']:.3e}) in {pre['gflat_slices_before_fold']}")
        if pre["shadow_nonzero_before_fold"] == 0:
            bad.append(f"{step}: the fixed-point shadow is empty after the backward")
        if pre["gflat_nonzero_after_fold"] == 0:
            bad.append(f"{step}: the fp32 gradients are zero after the fold")
        if pre["shadow_nonzero_after_fold"] != 0:
            bad.append(f"{step}: the fold left {pre['shadow_nonzero_after_fold']} shadow entries")
        field.zero_grad_fused()

    def ray_static():
        o = st(cr, ct, None, gx, gz, gv, ray_type="ndc")
        ((o[6] * w_rgb).sum() + (o[7] * w_ns[0]).sum() + (o[4] * w_ns[1]).sum()).backward()

    def ray_dynamic():
        o = dy(cr, ct, None, gx, gz, gv, ray_type="ndc")
        ((o[6] * w_rgb).sum() + (o[7] * w_ns[0]).sum() + (o[4] * w_ns[1]).sum() + (o[2] * w_ns[2]).sum()).backward()

    ray_static()
    check("ray static", st)
    ray_dynamic()
    check("ray dynamic", dy)
    L.set_scatter_mode("sorted")
    try:
        ray_dynamic()
        check("ray dynamic, sorted scatter", dy)
    finally:
        L.set_scatter_mode("auto")
    (st.compute_densityfeature(xn, tm, None).sum() + (st.compute_appfeature(xn, tm, None) * w_rgb.reshape(-1)[:M * 27].reshape(M, 27)).sum()).backward()
    check("features static", st)
    (dy.compute_densityfeature(xn, tm, None).sum() + dy.compute_blendingfeature(xn, tm, None).sum()
     + (dy.compute_appfeature(xn, tm, None) * w_rgb.reshape(-1)[:M * 27].reshape(M, 27)).sum()
     + (dy.warp_coordinate(dy.unnormalize_coord(xn), tm) * w_rgb.reshape(-1, 3)[:M]).sum()).backward()
    check("features dynamic", dy)
    sf_f, sf_b = dy.get_forward_backward_scene_flow(gx, ct)
    ((sf_f * w_rgb).sum() + (sf_b * w_rgb.flip(0)).sum()).backward()
    check("scene flow", dy)
    assert not bad, "\n".join(bad)
    return report


def test_every_gradient_addition_reaches_the_fixed_point_shadow(tmp_path):
    report = run_twin(tmp_path, [CHILD, "case", "test_gpu_det_binding"], det=True)
    print("\n".join(json.dumps(r) for r in report))
    assert len(report) == 6, report
