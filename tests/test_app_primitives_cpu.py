"""No GPU: the float64 references of tests/_app_prim.py (the backward-data kernels of the appearance phase) against torch autograd of
the appearance MLPs written out here from their formulas; a float32 evaluation in the kernels' order against every bound the GPU
file uses; the power of the generated inputs against eight planted defects; the describe layouts against each other."""
import os
import sys

import numpy as np
import pytest
import torch

from _util import pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _app_prim as Q   # noqa: E402

f64 = np.float64


_LAY = {}


def _lay(field):
    if field not in _LAY:
        _LAY[field] = Q.layout(pkg(), field)
    return _LAY[field]


CASES = Q.cpu_cases()
IDS = [f"{c['field']}-{c['mode']}-{c['N']}x{c['S']}-{c['count']}-{c['ray_type']}" for c in CASES]


def test_entry_points_are_declared_and_sized():
    L = pkg()
    for name in ("rdrf_selftest_app_bwd", "rdrf_selftest_app_describe", "rdrf_selftest_app_bwd_workspace_bytes"):
        assert name in L.SIGNATURES and hasattr(L.lib, name)
        assert name in open(os.path.join(ROOT, "include", "rodynrf.h")).read()
    assert L.lib.rdrf_selftest_app_bwd_workspace_bytes(1, 1) == L.lib.rdrf_selftest_app_bwd_workspace_bytes(4096, 115) > 0


def test_describe_agrees_with_the_other_describes():
    L = pkg()
    for field in Q.FIELDS:
        lay = _lay(field)   # its assertions: the dz1 job's rows, the P row order, the scatter's first DA row and record size
        dyn = field == "dyn"
        assert lay["grows"] == 544 and lay["rows"] == (640 if dyn else 544) and lay["rec"] == (216 if dyn else 0)
        assert [lay[k] for k in ("DZV", "DZ2", "DZ1", "DF", "DA")] == sorted(lay[k] for k in ("DZV", "DZ2", "DZ1", "DF", "DA"))
        assert lay["DA"] + 2 * lay["nda"] <= lay["grows"] and lay["ncomp"] == (216 if dyn else 72)
        assert sum(n for _, n in lay["unread"]) + 256 + (64 if dyn else 128) == lay["rows"]
        if dyn:   # a record holds every component once
            offs = sorted(o + i for _, o in lay["quads"] for i in range(4))
            assert offs == list(range(216))
        # the dz rows of the other products of the plan start where this describe says
        import _dw_prim as DW
        plan = {"dyn": "DYN_APP", "fea": "STATIC_FEA", "te": "STATIC_TE"}[field]
        a_rows = {j["A_row0"] for j in DW.describe(L, plan, 0)["jobs"]}
        assert a_rows == {lay["DZV"], lay["DZ2"], lay["DZ1"], lay["DF"]}


def test_geometry_of_the_large_shapes():
    """the smallest tile counts with several waves per workgroup and with waves that take a second tile from the queue"""
    L = pkg()
    for field in Q.FIELDS:
        t_waves, t_walk = Q.large_tiles(L, field)
        assert t_waves < t_walk <= 2050
        for t, walk in ((t_waves, False), (t_walk, True)):
            g = Q.app_describe(L, field, "rows", t * 32, 1)
            assert g["tiles"] == t and g["waves"] > 1 and (t > g["grid"] * g["waves"]) == walk
            g = Q.app_describe(L, field, "rows", (t - 1) * 32, 1)
            assert (g["waves"] == 1) if not walk else (t - 1 <= g["grid"] * g["waves"])


def test_errors_of_describe():
    import ctypes as C
    L = pkg()
    buf = (C.c_int * 16)()
    assert L.lib.rdrf_selftest_app_describe(3, 0, 1, 1, buf, 16) == -1
    assert L.lib.rdrf_selftest_app_describe(0, 3, 1, 1, buf, 16) == -1
    assert L.lib.rdrf_selftest_app_describe(0, 0, 1, 0, buf, 16) == -1
    assert L.lib.rdrf_selftest_app_describe(0, 0, 1, 1, buf, 15) == -3


# ---- autograd ------------------------------------------------------------------------------------------------------------------
def _pe(x, freqs):
    """sin then cos of x[..., d] 2^k at index d * freqs + k"""
    p = (x[..., None] * (2.0 ** torch.arange(freqs, dtype=x.dtype))).reshape(x.shape[:-1] + (freqs * x.shape[-1],))
    return torch.cat([torch.sin(p), torch.cos(p)], -1)


def _autograd_case(field, mode, ray_type, n=37, N=5, S=11, seed=0):
    """a consistent float64 forward of the field's appearance MLP; -> (case with float64 rows, weights, autograd results)"""
    lay = _lay(field)
    dyn = field == "dyn"
    W32 = Q.app_weights(field, seed)
    W = {k: torch.from_numpy(v.astype(f64)) for k, v in W32.items()}
    g = torch.Generator().manual_seed(100 + seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)   # noqa: E731
    b1, b2 = rn(128) * 0.3, rn(128) * 0.3
    c = Q.app_case(field, mode, N, S, n, ray_type, seed)
    idx = torch.from_numpy(c["list"][:n].astype(np.int64))
    A = rn(n, lay["ncomp"]).requires_grad_()
    rays_d = torch.from_numpy(c["rays"][:, 3:6].astype(f64)).requires_grad_()
    d = rays_d[idx // S]
    vd = d / d.norm(dim=-1, keepdim=True) if ray_type in ("ndc", "contract") else d
    F = A @ W["basis"].T
    F.retain_grad()
    if dyn:   # MLP_Fea_late_view, feape 0, viewpe 0: [features, pts, PE(pts, 10), time, PE(time, 8)]; the view direction detached
        xn = (torch.rand(n, 3, generator=g, dtype=torch.float64) * 2 - 1).requires_grad_()
        t = torch.rand(n, 1, generator=g, dtype=torch.float64) * 2 - 1
        X = torch.cat([F, xn, _pe(xn, 10), t, _pe(t, 8)], -1)
        tail = vd.detach()
    elif field == "fea":   # MLP_Fea, feape 2, viewpe 0: [features, viewdirs, PE(features, 2)], three plain layers
        X = torch.cat([F, vd, _pe(F, 2)], -1)
        tail = None
    else:   # MLP_Fea_TimeEmbedding, feape 2, viewpe 0: [features, PE(features, 2)]; the view direction joins the output layer
        X = torch.cat([F, _pe(F, 2)], -1)
        tail = vd
    z1 = X @ W["w1"].T + b1
    H1 = torch.relu(z1)
    z2 = H1 @ W["w2"].T + b2
    H2 = torch.relu(z2)
    v = (H2 if tail is None else torch.cat([H2, tail], -1)) @ W["w3"].T + W["b3"]
    for x in (z1, z2, v):
        x.retain_grad()
    g_rgb = torch.from_numpy(c["g_rgb"].astype(f64))
    (torch.sigmoid(v) * g_rgb[idx]).sum().backward()
    icol = np.array(lay["icol"])
    if dyn:
        icol[3] = 90
    Xn = X.detach().numpy()
    c["H1"], c["H2"] = H1.detach().numpy(), H2.detach().numpy()
    c["IN"] = np.where(icol[None, :] >= 0, Xn[:, np.maximum(icol, 0)], 0.0)
    got = dict(dzv=v.grad, dz2=z2.grad, dz1=z1.grad, dF=F.grad, dA=A.grad, g_rays=rays_d.grad)
    if dyn:
        got["dxn"] = xn.grad
    return c, W32, {k: (None if x is None else x.numpy()) for k, x in got.items()}


@pytest.mark.parametrize("field,mode,ray_type", [("dyn", "rows", "ndc"), ("dyn", "rec", "other")]
                         + [(f, "rows", rt) for f in ("fea", "te") for rt in Q.RAY_TYPES])
def test_reference_equals_autograd(field, mode, ray_type):
    lay = _lay(field)
    c, W, want = _autograd_case(field, mode, ray_type)
    ref = Q.app_reference(c, W, lay)

    def close(name, a, b, cond):
        err = np.abs(a - b).max()
        assert err <= 1e-12 * max(cond, 1e-300), f"{name}: {err:.3e} against a condition scale of {cond:.3e}"

    for k in ("dzv", "dz2", "dz1"):
        close(k, ref[k][0], want[k], np.abs(want[k]).max())
    dF = ref["dF"][0]
    close("dF", dF[:, :27], want["dF"], np.abs(want["dF"]).max())
    assert (dF[:, 27:] == 0).all()
    dA = ref["dA"][0]
    close("dA", dA[:, :lay["ncomp"]], want["dA"], np.abs(want["dA"]).max())
    assert (dA[:, lay["ncomp"]:] == 0).all()
    if field == "dyn":
        close("dxn", ref["dxn"][0], want["dxn"], np.abs(want["dxn"]).max())
        assert want["g_rays"] is None or not want["g_rays"].any()   # late_view detaches the view direction
        if mode == "rec":
            for e0, off in lay["quads"]:
                assert np.array_equal(ref["rec"][0][:, off:off + 4], dA[:, e0:e0 + 4])
    else:
        close("g_rays", ref["g_rays"][0], want["g_rays"], np.abs(ref["g_rays_terms"][0]).sum())


def test_feature_mode_equals_autograd():
    for field in Q.FIELDS:
        lay = _lay(field)
        c = Q.app_case(field, "feat", 45, 1, 45)
        W = Q.app_weights(field)
        A = torch.zeros(45, lay["ncomp"], dtype=torch.float64, requires_grad=True)
        ((A @ torch.from_numpy(W["basis"].astype(f64)).T) * torch.from_numpy(c["g_feat"].astype(f64))).sum().backward()
        ref = Q.app_reference(c, W, lay)
        assert np.abs(ref["dA"][0][:, :lay["ncomp"]] - A.grad.numpy()).max() <= 1e-12 * np.abs(A.grad.numpy()).max()
        assert np.array_equal(ref["dF"][0][:, :27], c["g_feat"].astype(f64)) and (ref["dF"][1] == 0).all()


# ---- the bounds and the generators --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_float32_evaluation_fits_every_bound(c):
    lay = _lay(c["field"])
    W = Q.app_weights(c["field"], c["seed"])
    pre = np.random.default_rng(5).standard_normal((c["N"], 3)).astype(np.float32) if c["mode"] != "feat" else None
    ref, got = Q.app_reference(c, W, lay, pre_rays=pre), Q.app_eval32(c, W, lay, pre_rays=pre)
    for name in Q.compared(c):
        r = Q.ratio(got[name], ref[name][0], ref[name][1])
        assert r <= 1.0, f"{name}: a float32 evaluation sits at {r:.3f} of the bound"


def test_generated_rows_are_finite_and_hold_the_gate_values():
    for c in CASES:
        if c["mode"] == "feat" or c["count"] == 0:
            continue
        lay = _lay(c["field"])
        rows = Q.app_rows(c, lay)
        for key, n in (("H2", 128), ("H1", 128), ("IN", c["IN"].shape[1])):
            assert np.isfinite(rows[:c["T"], lay[key]:lay[key] + n, :]).all(), "every lane of a walked tile, padding included"
        for r0, n in lay["unread"]:
            assert np.isnan(rows[:, r0:r0 + n, :]).all()
        assert np.isnan(rows[c["T"]:]).all()
        if c["count"] >= 31:
            for key in ("H2", "H1"):
                bits = set(c[key][:c["count"]].view(np.uint32).ravel().tolist())
                assert {0x00000000, 0x80000000, 0x00800000} <= bits and (np.abs(c[key]) > 0.25).any()
        assert len(set(c["list"][:c["count"]].tolist())) == c["count"] and (c["list"][:c["count"]] < c["N"] * c["S"]).all()


@pytest.mark.parametrize("defect", sorted(Q.DEFECTS))
def test_planted_defects_exceed_the_bounds(defect):
    """on every generated case the defect concerns, at least one element of a compared output moves by 16 bounds or more"""
    seen = 0
    for c in CASES:
        if c["field"] not in Q.DEFECTS[defect] or c["mode"] == "feat" or c["count"] == 0:
            continue
        if defect == "rec_swap" and c["mode"] != "rec":
            continue
        if defect == "no_projection" and c["ray_type"] not in ("ndc", "contract"):
            continue
        lay = _lay(c["field"])
        W = Q.app_weights(c["field"], c["seed"])
        ref, bad = Q.app_reference(c, W, lay), Q.app_reference(c, W, lay, defect=defect)
        worst = max(Q.ratio(bad[name][0], ref[name][0], ref[name][1]) for name in Q.compared(c))
        assert worst >= Q.POWER, f"{defect} on {c['field']} {c['mode']} count {c['count']} {c['ray_type']}: only {worst:.2f} bounds"
        seen += 1
    assert seen >= 4
