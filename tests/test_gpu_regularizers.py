"""TV regulariser (utils.py:157-181, models/tensoRF.py:100-116, 418-444) through
the C ABI against vectors generated from the reference: values (NaN for lines, like the reference)
and gradients, plain autograd and fused accumulation, channel-last and contiguous storage."""
import os

import numpy as np
import pytest
import torch

from _util import assert_close, pkg

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(os.path.dirname(__file__), "golden", "tv.npz"))


@pytest.mark.parametrize("name", ["plane", "line", "row"])
@pytest.mark.parametrize("layout", ["contiguous", "channel_last"])
def test_tvloss_single_tensor_golden(name, layout):
    import rodynrf
    F = pkg("fields")
    tv = rodynrf.TVLoss()
    for ax in (None, "h", "w"):
        x = torch.from_numpy(G[f"t.{name}.x"]).clone().cuda()
        if layout == "channel_last":
            x = F.channel_last_(x)
        x.requires_grad_(True)
        v = tv(x, ax) if ax else tv(x)
        ref = G[f"t.{name}.v.{ax}"]
        assert bool(torch.isnan(v)) == bool(np.isnan(ref)), (name, ax)
        if not np.isnan(ref):
            assert_close(v, ref, f"tv {name} {ax}", rtol=2e-5)
        gx, = torch.autograd.grad(v, x)
        gref = G[f"t.{name}.g.{ax}"]
        assert np.array_equal(np.isnan(gref), torch.isnan(gx).cpu().numpy()), (name, ax)
        assert_close(torch.nan_to_num(gx), np.nan_to_num(gref), f"d tv {name} {ax}", rtol=2e-5)
        assert gx.stride() == x.stride()


@pytest.mark.parametrize("fused", [False, True])
def test_tv_family_golden(fused):
    import rodynrf
    from _gpu_util import fields_from_case
    _, st, dy, _ = fields_from_case("ndc_relu")
    tv = rodynrf.TVLoss()
    for tag, mod, fams in (("s", st, ("density", "app")), ("d", dy, ("density", "blending", "app"))):
        mod.fused_grad = fused
        if fused:
            mod.zero_grad_fused()
        tot = 0
        for fam in fams:
            t = getattr(mod, f"TV_loss_{fam}")(tv)
            assert bool(torch.isnan(t)) == bool(np.isnan(G[f"f.{tag}.{fam}.total"]))
            tot = tot + t
        tot.backward()
        for fam in fams:
            for kind in ("plane", "line"):
                for i, p in enumerate(getattr(mod, f"{fam}_{kind}")):
                    assert_close(p.grad, G[f"f.{tag}.{fam}.g.{fam}_{kind}.{i}"], f"{tag}.{fam}_{kind}.{i}", rtol=2e-5)


def test_tv_family_foreign_callable_matches():
    """a non-rodynrf `reg` callable is applied tensor by tensor, as in the reference"""
    import rodynrf
    from _gpu_util import fields_from_case
    from oracle import rodynrf_oracle as O
    _, st, _, _ = fields_from_case("ndc_relu")
    a = st.TV_loss_app(rodynrf.TVLoss())
    b = st.TV_loss_app(lambda x: O.tv_loss(x))
    ga = torch.autograd.grad(a, list(st.app_plane))
    gb = torch.autograd.grad(b, list(st.app_plane))
    for x, y in zip(ga, gb):
        assert_close(x, y, "tv app plane grad", rtol=2e-5)


def test_l1_and_ortho_regularisers_golden():
    """density_L1 / blending_L1 / vector_comp_diffs (models/tensoRF.py:63-98, 378-416) on the weights
    of the ndc_relu case against the reference's values and gradients."""
    from _gpu_util import fields_from_case
    _, st, dy, _ = fields_from_case("ndc_relu")
    for tag, mod, names in (("s", st, ("density_L1", "vector_comp_diffs")),
                            ("d", dy, ("density_L1", "blending_L1"))):
        for nm in names:
            val = getattr(mod, nm)()
            assert_close(val, G[f"r.{tag}.{nm}.value"], f"{tag}.{nm}", rtol=2e-5)
            fam = "blending" if nm == "blending_L1" else "density"
            ps = list(getattr(mod, f"{fam}_plane")) + list(getattr(mod, f"{fam}_line"))
            if nm == "vector_comp_diffs":
                ps = list(mod.density_line) + list(mod.app_line)
            gs = torch.autograd.grad(val, ps, allow_unused=True)
            for i, gg in enumerate(gs):
                ref = G[f"r.{tag}.{nm}.g{i}"]
                gg = torch.zeros_like(ps[i]) if gg is None else gg
                assert_close(gg, ref, f"{tag}.{nm}.g{i}", rtol=5e-5)
    assert not hasattr(dy, "vector_comp_diffs")


def test_tv_accumulate_grad_matches_autograd_path():
    """TVLoss.accumulate_grad_ (one launch, no value) adds exactly the gradient that TV_loss_* + backward give,
    for fused and plain gradient storage, with per-family weights."""
    import rodynrf
    from _gpu_util import fields_from_case
    g, st, dy, _ = fields_from_case("ndc_relu")
    tv = rodynrf.TVLoss()
    fams = [(dy.density_plane, dy.density_line), (dy.blending_plane, dy.blending_line), (dy.app_plane, dy.app_line)]
    wts = [0.7, 0.7, 0.2]
    (0.7 * (dy.TV_loss_density(tv) + dy.TV_loss_blending(tv)) + 0.2 * dy.TV_loss_app(tv)).backward()
    ref = [p.grad.clone() for pl, ln in fams for p in list(pl) + list(ln)]
    for fused in (False, True):
        for p in dy.parameters():
            p.grad = None
        dy.fused_grad = fused
        if fused:
            dy.zero_grad_fused()
        tv.accumulate_grad_(dy, fams, wts)
        tv.accumulate_grad_(dy, fams, wts)          # accumulates
        got = [p.grad for pl, ln in fams for p in list(pl) + list(ln)]
        for i, (a, b) in enumerate(zip(got, ref)):
            assert_close(a, 2 * b, f"fused={fused} tensor {i}", rtol=1e-5)
