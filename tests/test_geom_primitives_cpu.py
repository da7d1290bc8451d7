"""Keeps tests/_geom_prim.py honest without a GPU: every float64 reference there (and every hand-written adjoint) against the
oracle evaluated in float64 with torch autograd, to 1e-12 of the condition scale; the reference's own fixtures
(tests/golden/raygen.npz, induce_flow.npz: float32 vectors) inside the derived bounds; every generator produces the regime it
claims with every discrete decision safe; and the FLOAT32 oracle evaluation of every generated case lies inside the bounds
test_gpu_geom_primitives.py holds the kernels to, so that no bound is tighter than a legitimate float32 ordering."""
import os

import numpy as np
import pytest
import torch

import _geom_prim as G
from _geom_prim import F32, U, f64
from _util import GOLDEN, record_margin
from oracle import rodynrf_oracle as O

EPS64 = 1e-12


def _agree(ref, other, tag):
    """float64 forms agree to 1e-12 of the condition scale (the first-order bound over u, at least the value itself)"""
    other = f64(other).reshape(ref.v.shape)
    cond = np.maximum(ref.e / U, np.abs(ref.v))
    err = np.abs(ref.v - other)
    assert (err <= EPS64 * cond + 1e-300).all(), f"{tag}: float64 forms differ by {float((err / (cond + 1e-300)).max()):.2e} of the scale"


def _inside(got, ref, tag, skip=None):
    r = G.bound_ratio(got, ref, skip)
    record_margin(tag, r)
    assert r <= 1.0, f"{tag}: the float32 evaluation sits at {r:.3f} of the bound"
    return r


def _t(a, dt, rg=False):
    return None if a is None else torch.from_numpy(np.asarray(a)).to(dt).requires_grad_(rg)


# ---- ray generation ---------------------------------------------------------------------------------------------------------
def _raygen_oracle(c, dt, g=True):
    poses, focal = _t(c["poses"], dt, True), _t(np.asarray(c["focal"]).reshape(()), dt, True)
    rays = O.generate_rays(torch.from_numpy(c["ids"]), poses, focal, c["H"], c["W"], c["ndc"], c["near"], _t(c["uv"], dt), c["view_shift"])
    if not g:
        return rays.detach()
    gp, gf = torch.autograd.grad((rays * _t(c["g"], dt)).sum(), [poses, focal])
    return rays.detach(), _t(c["pre_p"], dt) + gp, _t(c["pre_f"], dt) + gf.reshape(1)


RAYGEN_CASES = G.raygen_cases()


def test_raygen_reference_is_the_oracle_with_autograd_in_float64():
    for tag, k in RAYGEN_CASES:
        if k["N"] != 257:
            continue
        c = G.raygen_case(**k)
        with G.exact_consts():
            r = G.raygen_ref(c["ids"], c["uv"], c["view_shift"], c["poses"], c["focal"], c["H"], c["W"], c["ndc"], c["near"], c["g"],
                             c["pre_p"], c["pre_f"])
        rays, gp, gf = _raygen_oracle(c, torch.float64)
        _agree(r["rays"], rays, tag + " rays")
        _agree(r["g_poses"], gp, tag + " g_poses")
        _agree(r["g_focal"], gf, tag + " g_focal")


def test_raygen_fixture_inside_bound():
    """tests/golden/raygen.npz (the reference's own float32 rays, NDC and world)"""
    z = np.load(os.path.join(GOLDEN, "raygen.npz"))
    for ndc, key in ((True, "rays"), (False, "rays_world")):
        r = G.raygen_ref(z["ids"], None, 0, z["poses"], float(z["focal"]), int(z["H"]), int(z["W"]), ndc, 1.0)
        assert r["rays"].r.max() <= G.RHO_ORDINARY
        _inside(z[key], r["rays"], f"raygen fixture {key}")


@pytest.mark.parametrize("tag,k", RAYGEN_CASES, ids=[t for t, _ in RAYGEN_CASES])
def test_raygen_generators_and_float32_inside_bound(tag, k):
    c = G.raygen_case(**k)
    ref = c["ref"]
    assert G.margins_ok(c["margins"]) and max(ref[n].r.max() for n in ("rays", "g_poses", "g_focal")) <= G.RHO_ORDINARY
    assert np.isfinite(ref["g_poses"].e).all() and np.isfinite(ref["rays"].e).all()
    assert c["pre_p"].all() and c["pre_f"].all() and c["g"][c["eff"] != c["dead"]].all()
    nrm = np.linalg.norm(f64(c["poses"])[:, :3], axis=-1)
    if k["T"] >= 5:
        assert nrm.min() < 0.5 and nrm.max() > 2.0, "rows are not normalised"
    if k.get("ids_mode") == "big":
        assert c["ids"].max() > 2 ** 31
    if k.get("ids_mode") == "ends" and k.get("view_shift", 0):
        assert set(np.unique(c["eff"])) == {min(max(0 + k["view_shift"], 0), 4), min(max(4 + k["view_shift"], 0), 4)}
    if k.get("poses") == "skew":
        p = f64(c["poses"])
        cos = (p[:, :3] * p[:, 3:6]).sum(-1) / nrm / np.linalg.norm(p[:, 3:6], axis=-1)
        assert (np.degrees(np.arccos(np.clip(cos, -1, 1))) < 8).all()
    if c["dead"] >= 0:
        assert (ref["g_poses"].v[c["dead"]] == f64(c["pre_p"])[c["dead"]]).all()
    rays, gp, gf = _raygen_oracle(c, torch.float32)
    _inside(rays, ref["rays"], tag + " rays")
    _inside(gp, ref["g_poses"], tag + " g_poses")
    _inside(gf, ref["g_focal"], tag + " g_focal")


def test_raygen_near_singular_set():
    c = G.raygen_singular_case()
    ref = c["ref"]
    skip = ref["rays"].r > G.RHO_LIMIT
    assert 0 < skip.mean() <= 1 / 8, f"{skip.mean():.3f} of the elements fall back to the finiteness check"
    assert np.abs(ref["dz"].v).min() < 1e-4 and np.abs(ref["dz"].v).max() > 1e-2
    skip_p = ref["g_poses"].r > G.RHO_LIMIT
    assert 0 < skip_p.mean() <= 1 / 8, f"{skip_p.mean():.3f} of the g_poses elements fall back to the finiteness check"
    assert len(np.unique(ref["view"])) == len(ref["view"]) == c["T"], "one ray per view: a row carries its own ray's divisor bound"
    rays, gp, gf = _raygen_oracle(c, torch.float32)
    _inside(rays, ref["rays"], "raygen near-singular rays", skip)
    _inside(gp, ref["g_poses"], "raygen near-singular g_poses", skip_p)
    # g_focal sums every ray, the over-limit ones included: finiteness only on this set
    assert (ref["g_focal"].r > G.RHO_LIMIT).all() and np.isfinite(f64(rays)).all() and np.isfinite(f64(gf)).all()


# ---- samplers ---------------------------------------------------------------------------------------------------------------
def _world_torch(rays, S, near, far, step, jitter, box, eps=1e-6):
    """TensorBase.sample_ray in torch (the world-space march the oracle does not restate)"""
    o, d = rays[:, :3], rays[:, 3:]
    vec = torch.where(d == 0, torch.full_like(d, eps), d)
    ra, rb = (box[1] - o) / vec, (box[0] - o) / vec
    t_min = torch.minimum(ra, rb).amax(-1).clamp(min=near, max=far)
    rngv = torch.arange(S, dtype=rays.dtype)[None].repeat(rays.shape[0], 1)
    if jitter is not None:
        rngv = rngv + jitter[:, None]
    z = t_min[:, None] + step * rngv
    pts = o[:, None] + d[:, None] * z[..., None]
    return pts, z, ~((box[0] > pts) | (pts > box[1])).any(-1)


def _sampler_oracle(c, dt):
    rays = _t(c["rays"], dt)
    nf = [float(F32(c["near"])), float(F32(c["far"]))]
    if c["kind"] == "world":
        return _world_torch(rays, c["S"], nf[0], nf[1], float(F32(c["step"])), _t(c["jitter"], dt), _t(c["box"], dt),
                            1e-6 if dt == torch.float64 else float(F32(1e-6)))
    old = torch.get_default_dtype()
    torch.set_default_dtype(dt)
    try:
        return O.sampleXYZ(rays, _t(c["box"], dt), nf, c["S"], c["kind"], _t(c["jitter"], dt), _t(c.get("jout"), dt))
    finally:
        torch.set_default_dtype(old)


def _sampler_ref(c):
    if c["kind"] == "ndc":
        return G.sample_ndc_ref(c["rays"], c["S"], c["near"], c["far"], c["jitter"], c["box"])
    if c["kind"] == "contract":
        return G.sample_contract_ref(c["rays"], c["S"], c["near"], c["far"], c["jitter"], c["jout"])
    return G.sample_world_ref(c["rays"], c["S"], c["near"], c["far"], c["step"], c["jitter"], c["box"])


@pytest.mark.parametrize("kind", ["ndc", "contract", "world"])
def test_sampler_references_generators_and_float32_inside_bound(kind):
    near_face = total = 0
    for tag, k in G.sampler_cases():
        if k["kind"] != kind:
            continue
        c = G.sampler_case(**k)
        ref = c["ref"]
        assert G.margins_ok(c["margins"]) and np.isfinite(ref["xyz"].e).all()
        with G.exact_consts():
            r64 = _sampler_ref(c)
        xyz, z, valid = _sampler_oracle(c, torch.float64)
        _agree(r64["xyz"], xyz, tag + " xyz")
        _agree(r64["z"], z, tag + " z")
        assert np.array_equal(valid.numpy(), r64["valid"])
        xyz, z, valid = _sampler_oracle(c, torch.float32)
        _inside(xyz, ref["xyz"], tag + " xyz")
        _inside(z, ref["z"], tag + " z")
        clear = ref["clear"] > 0
        assert np.array_equal(valid.numpy()[clear], ref["valid"][clear]), tag
        assert int((~clear).sum()) * 50 <= clear.size, f"{tag}: {int((~clear).sum())} of {clear.size} samples lie within their bound of a face"
        near_face += int((~clear).sum())
        total += clear.size
        if kind == "contract":
            assert ref["big"].any() and (k["S"] < 3 or not ref["big"].all()), "samples on both sides of nrm = 1"
    assert near_face * 50 <= total, f"{near_face} of {total} samples lie within their bound of a face"
    if kind == "contract":
        c = G.contract_exact_case()
        xyz, z, _ = _sampler_oracle(c, torch.float32)
        r = _sampler_ref(c)
        assert np.array_equal(f64(z)[:, :4], np.tile(c["z_inner"], (2, 1))) and np.array_equal(r["z"].v[:, :4], f64(z)[:, :4])
        assert np.array_equal(f64(xyz)[:, :2], c["pts_inner"]) and np.array_equal(r["xyz"].v[:, :2], c["pts_inner"])
        assert (np.abs(c["pts_inner"]).max(-1) < 1).all()
    if kind != "contract":
        c = G.on_face_case(kind)
        r = _sampler_ref(c)
        assert (r["xyz"].e[c["expect"]] >= 0).all() and np.array_equal(r["valid"], c["expect"])
        lo, hi = f64(c["box"])
        on = ((r["xyz"].v == lo) | (r["xyz"].v == hi)).any(-1)
        assert on[c["expect"]].sum() >= 6, "the on-face set holds points exactly on a face"
        xyz, _, valid = _sampler_oracle(c, torch.float32)
        assert np.array_equal(f64(xyz), r["xyz"].v) and np.array_equal(valid.numpy(), c["expect"]), "exactly representable"


def test_world_sampler_rows():
    c = G.sample_world_bwd_case(5)
    tm = c["ref"]["tmin"]
    R = c["rays"]
    assert [int(a) for a in tm["axis"][:6]] == [0, 0, 1, 1, 2, 2] and [bool(u) for u in tm["upper"][:6]] == [False, True] * 3
    assert tm["raw"].v[6] < 0.5 and tm["raw"].v[7] > 6.0 and tm["raw"].v[8] == 0.5 and tm["through"][8]
    assert not tm["through"][6] and not tm["through"][7] and tm["through"][:6].all()
    for k in range(3):
        assert R[9 + k, 3 + k] == 0 and tm["axis"][9 + k] == k and not tm["through"][9 + k]
    z = G.sample_world_bwd_zero_case(5)
    assert z["ref"]["tmin"]["through"].all() and [int(a) for a in z["ref"]["tmin"]["axis"]] == [0, 1, 2]


# ---- sampler adjoints -------------------------------------------------------------------------------------------------------
def _sample_bwd_oracle(c, dt):
    rays = _t(c["rays"], dt, True)
    z = _t(c["z"], dt)
    pts = rays[:, None, :3] + rays[:, None, 3:] * z[..., None]
    if c["kind"] == "contract":
        pts = O._linf_contract(pts)
    g, = torch.autograd.grad((pts * _t(c["g"], dt)).sum(), rays)
    return _t(c["pre"], dt) + g


@pytest.mark.parametrize("kind", ["ndc", "contract"])
def test_sample_bwd_reference_generators_and_float32_inside_bound(kind):
    seen = set()
    for S in G.SAMPLE_BWD_S:
        for N in (1, 3, 6):
            c = G.sample_bwd_case(kind, N, S)
            tag = f"sample_bwd {kind} N={N} S={S}"
            assert G.margins_ok(c["margins"])
            _agree(c["ref"]["g_rays"], _sample_bwd_oracle(c, torch.float64), tag)
            _inside(_sample_bwd_oracle(c, torch.float32), c["ref"]["g_rays"], tag)
            if kind == "contract":
                p = f64(c["rays"])[:, None, :3] + f64(c["rays"])[:, None, 3:] * f64(c["z"])[..., None]
                big = np.abs(p).max(-1) > 1
                k = np.abs(p).argmax(-1)
                seen |= {(int(a), bool(s)) for a, s in zip(k[big], np.take_along_axis(p, k[..., None], -1)[..., 0][big] > 0)}
                if S >= 63:
                    assert big.any() and not big.all()
    if kind == "contract":
        c = G.sample_bwd_case(kind, 6, 64)
        p = f64(c["rays"])[:, None, :3] + f64(c["rays"])[:, None, 3:] * f64(c["z"])[..., None]
        k = np.abs(p).argmax(-1)
        big = np.abs(p).max(-1) > 1
        seen = {(int(a), bool(s)) for a, s in zip(k[big], np.take_along_axis(p, k[..., None], -1)[..., 0][big] > 0)}
        assert seen == {(a, s) for a in range(3) for s in (False, True)}, "arg-max on every axis with both signs (N = 6)"


def _world_bwd_oracle(c, dt):
    rays = _t(c["rays"], dt, True)
    box = _t(c["box"], dt)
    o, d = rays[:, :3], rays[:, 3:]
    vec = torch.where(d == 0, torch.full_like(d, 1e-6 if dt == torch.float64 else float(F32(1e-6))), d)
    t_min = torch.minimum((box[1] - o) / vec, (box[0] - o) / vec).amax(-1).clamp(min=float(F32(c["near"])), max=float(F32(c["far"])))
    z0 = _t(c["z"], dt)
    z = z0 + (t_min - t_min.detach())[:, None]            # the stored depths, differentiable through t_min
    pts = o[:, None] + d[:, None] * z[..., None]
    loss = 0
    if c["g"] is not None:
        loss = loss + (pts * _t(c["g"], dt)).sum()
    if c["gz"] is not None:
        loss = loss + (z * _t(c["gz"], dt)).sum()
    g, = torch.autograd.grad(loss, rays)
    return _t(c["pre"], dt) + g


def test_sample_world_bwd_reference_generators_and_float32_inside_bound():
    for S in G.SAMPLE_BWD_S:
        cases = [(m, G.sample_world_bwd_case(S, m)) for m in ("both", "xyz", "z")] + [("d == 0 selected", G.sample_world_bwd_zero_case(S))]
        for m, c in cases:
            tag = f"sample_world_bwd S={S} {m}"
            assert G.margins_ok(c["margins"])
            with G.exact_consts():
                r64 = G.sample_world_bwd_ref(c["rays"], c["z"], c["near"], c["far"], c["box"], c["g"], c["gz"], c["pre"])
            _agree(r64["g_rays"], _world_bwd_oracle(c, torch.float64), tag)
            _inside(_world_bwd_oracle(c, torch.float32), c["ref"]["g_rays"], tag)


# ---- induced flow -----------------------------------------------------------------------------------------------------------
def _flow_oracle(c, dt, fwd_only=False):
    rt = "contract" if c["contract"] else "ndc"
    N = c["w"].shape[0]
    ins = [_t(np.asarray(c["focal"]).reshape(()), dt, True), _t(c["c2w"], dt, True), _t(c["w"], dt, True), _t(c["pts"], dt, True),
           _t(c["rays"], dt, True)]
    flow, disp = O.induce_flow(c["H"], c["W"], ins[0], ins[1], ins[2], ins[3], _t(c["p2d"], dt), ins[4], rt)
    out = dict(flow=flow.detach(), disp=disp.detach().reshape(N))
    if fwd_only:
        return out
    loss = 0
    if c["g_flow"] is not None:
        loss = loss + (flow * _t(c["g_flow"], dt)).sum()
    if c["g_disp"] is not None:
        loss = loss + (disp.reshape(N) * _t(c["g_disp"], dt)).sum()
    gs = torch.autograd.grad(loss, ins)
    pre = c["pre"]
    for name, g in zip(("g_focal", "g_c2w", "g_weights", "g_pts", "g_rays"), gs):
        p = pre.get(name) if pre else None
        g = g.reshape(1) if name == "g_focal" else (g.reshape(N, 12) if name == "g_c2w" else g)
        out[name] = g if p is None else _t(p, dt).reshape(g.shape) + g
    return out


def _flow_ref(c):
    return G.flow_ref(c["H"], c["W"], c["focal"], c["c2w"], c["w"], c["pts"], c["p2d"], c["rays"], c["contract"], c["g_flow"], c["g_disp"],
                      c["pre"])


FLOW_CASES = G.flow_cases()


@pytest.mark.parametrize("tag,k", FLOW_CASES, ids=[t for t, _ in FLOW_CASES])
def test_flow_reference_generators_and_float32_inside_bound(tag, k):
    c = G.flow_case(**k)
    ref = c["ref"]
    assert G.margins_ok(c["margins"])
    assert max(ref[n].r.max() for n in ("flow", "disp") + G.FLOW_OUTS) <= G.RHO_ORDINARY, "no ray is masked out of the ordinary sets"
    assert all(np.isfinite(ref[n].e).all() for n in ("flow", "disp") + G.FLOW_OUTS)
    rows, acc = c["rows"], ref["acc"].v
    for n, kind in enumerate(rows):
        if kind == "zero weights":
            assert acc[n] == 0
        if kind == "unit weights":
            assert abs(acc[n] - 1) < 1e-6
        if kind == "P.z < -1":
            assert ref["P"][2].v[n] < -1 and ref["clamped"][n] and ref["gP"][2].v[n] == 0 and ref["gP"][2].e[n] == 0
        if kind in ("P.z > 1 - 1e-6", "zero weights") and not c["contract"]:
            assert ref["P"][2].v[n] > G.clamp_hi() and ref["clamped"][n] and ref["gP"][2].v[n] == 0
        if kind == "wn <= 1":
            assert max(abs(ref["P"][i].v[n]) for i in range(3)) <= 1
        if kind == "plain" and c["contract"]:
            assert max(abs(ref["P"][i].v[n]) for i in range(3)) > 1
        if kind == "zero direction":
            assert not c["rays"][n, 3:].any() and np.abs(c["rays"][n, :3]).max() < 1
    with G.exact_consts():
        r64 = _flow_ref(c)
    o64 = _flow_oracle(c, torch.float64)
    o32 = _flow_oracle(c, torch.float32)
    for name in ("flow", "disp") + G.FLOW_OUTS:
        _agree(r64[name], o64[name], f"{tag} {name}")
        _inside(o32[name], ref[name], f"{tag} {name}")


@pytest.mark.parametrize("rt", ["ndc", "contract"])
def test_flow_fixture_inside_bound(rt):
    """tests/golden/induce_flow.npz: the reference's own float32 flow, disparity and autograd gradients"""
    z = np.load(os.path.join(GOLDEN, "induce_flow.npz"))
    g = lambda k: z[f"{rt}.{k}"]
    N = g("weights").shape[0]
    r = G.flow_ref(int(z[f"{rt}.H"]), int(z[f"{rt}.W"]), float(g("focal")), g("c2w"), g("weights"), g("pts"), g("pts_2d"), g("rays"),
                   rt == "contract", g("lw_flow"), g("lw_disp").reshape(N))
    ok = np.maximum(r["flow"].r.max(-1), r["disp"].r) <= G.RHO_LIMIT
    assert ok.mean() > 0.9
    col = lambda a: ~ok.reshape(-1, *([1] * (a.ndim - 1))) & np.ones(a.shape, bool)
    for name, key in (("flow", "flow"), ("disp", "disp"), ("g_weights", "g_weights"), ("g_pts", "g_pts"), ("g_rays", "g_rays"),
                      ("g_c2w", "g_c2w")):
        _inside(g(key).reshape(r[name].v.shape), r[name], f"flow fixture {rt} {name}", col(r[name].v))
    if ok.all():
        _inside(g("g_focal").reshape(1), r["g_focal"], f"flow fixture {rt} g_focal")


@pytest.mark.parametrize("contract", [False, True])
def test_flow_near_singular_set(contract):
    c = G.flow_case(contract, 128, 13, singular=True)
    ref = c["ref"]
    assert G.margins_ok(c["margins"])
    o32 = _flow_oracle(c, torch.float32)
    for name in ("flow", "disp", "g_weights", "g_pts", "g_rays", "g_c2w"):
        skip = ref[name].r > G.RHO_LIMIT
        assert 0 < skip.mean() <= 1 / 8, f"{name}: {skip.mean():.3f} of the elements fall back to the finiteness check"
        _inside(o32[name], ref[name], f"flow near-singular {'contract' if contract else 'ndc'} {name}", skip)
    # g_focal sums every ray, the over-limit ones included: finiteness only on this set
    assert (ref["g_focal"].r > G.RHO_LIMIT).all() and np.isfinite(f64(o32["g_focal"])).all()
