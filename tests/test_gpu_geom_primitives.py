"""The ray geometry kernels on inputs of their own, against the float64 references of tests/_geom_prim.py: k_generate_rays and
k_generate_rays_bwd, k_sample_ndc / k_sample_contract / k_sample_world, k_sample_bwd, k_sample_world_bwd, k_induce_flow and
k_induce_flow_bwd (csrc/rdrf_misc.hip, csrc/rdrf_misc_dev.hpp).  Forward passes through rodynrf.generate_rays and rodynrf.sampleXYZ;
every adjoint and the induced flow through the C ABI, where the edges are (pre-filled accumulators, null pointers).

EVERY comparison is |err| <= bound element by element, the bound propagated operation by operation in tests/_geom_prim.py
(first-order running bounds, SECOND = 2 for the dropped second-order terms, arbitrary-order depth for the atomic sums, half an
ulp for stored sums), or an exact comparison (torch.equal / np.array_equal): `valid` against the box test of the kernel's own
points, points on a face, untouched accumulators, the zero subgradient of the clamp.  No ray is masked out except in the two
near-singular sets, where elements whose divisor bound exceeds RHO_LIMIT are checked for finiteness only.  The float32 oracle
meets the same bounds on the same cases (test_geom_primitives_cpu.py); profiles/geom_kernels_margins.txt holds both sets of ratios
and the mutation table."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import _geom_prim as G
from _util import pkg, record_margin

pytestmark = pytest.mark.gpu


def _cu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _check(got, ref, tag, skip=None):
    ratio = G.bound_ratio(got, ref, skip)
    record_margin(tag, ratio)
    assert ratio <= 1.0, f"{tag}: |err| is {ratio:.3f} x the propagated bound"


# ---- ray generation ---------------------------------------------------------------------------------------------------------
def _raygen_fwd(c):
    import rodynrf
    return rodynrf.generate_rays(_cu(c["ids"]), _cu(c["poses"]), _cu(np.asarray(c["focal"]).reshape(1)), c["H"], c["W"], ndc=c["ndc"],
                                 near=c["near"], uv=_cu(c["uv"]), view_shift=c["view_shift"])


def _raygen_bwd(c, g):
    L = pkg()
    ids, uv, poses, focal = _cu(c["ids"]), _cu(c["uv"]), _cu(c["poses"]), _cu(np.asarray(c["focal"]).reshape(1))
    gp, gf, tg = _cu(c["pre_p"]), _cu(c["pre_f"]), _cu(g)
    L.check(L.lib.rdrf_generate_rays_uv_bwd(L.ptr(ids), L.ptr(uv), c["view_shift"], L.ptr(poses), L.ptr(focal), len(c["ids"]), c["T"],
                                            c["H"], c["W"], int(c["ndc"]), c["near"], L.ptr(tg), L.ptr(gp), L.ptr(gf), L.stream_of(gp)),
            "generate_rays_bwd")
    return gp, gf


RAYGEN_CASES = G.raygen_cases()


@pytest.mark.parametrize("tag,k", RAYGEN_CASES, ids=[t for t, _ in RAYGEN_CASES])
def test_generate_rays_and_adjoint_match_float64(tag, k):
    """rays, and g_poses / g_focal ACCUMULATED onto non-zero pre-fills, across workgroups (N > 256), on both sides of
    GRB_LDS_POSES, with all ids on one view, clamped view shifts, ids above 2^31, un-normalised and skew 6-D rows, far-outside uv"""
    c = G.raygen_case(**k)
    ref = c["ref"]
    _check(_raygen_fwd(c), ref["rays"], tag + " rays")
    gp, gf = _raygen_bwd(c, c["g"])
    _check(gp, ref["g_poses"], tag + " g_poses")
    _check(gf, ref["g_focal"], tag + " g_focal")
    if c["dead"] >= 0:
        assert torch.equal(gp[c["dead"]].cpu(), torch.from_numpy(c["pre_p"][c["dead"]])), f"{tag}: a view whose rays have g_rays == 0"
    gp, gf = _raygen_bwd(c, np.zeros_like(c["g"]))
    assert torch.equal(gp.cpu(), torch.from_numpy(c["pre_p"])) and torch.equal(gf.cpu(), torch.from_numpy(c["pre_f"])), \
        f"{tag}: g_rays == 0 everywhere must leave the pre-filled g_poses and g_focal bit-identical"


def test_generate_rays_near_singular_set():
    c = G.raygen_singular_case()
    ref = c["ref"]
    _check(_raygen_fwd(c), ref["rays"], "raygen near-singular rays", ref["rays"].r > G.RHO_LIMIT)
    gp, gf = _raygen_bwd(c, c["g"])
    _check(gp, ref["g_poses"], "raygen near-singular g_poses", ref["g_poses"].r > G.RHO_LIMIT)   # one ray per view: own rows only
    assert bool(torch.isfinite(gf).all())   # g_focal sums every ray, the over-limit ones included: finiteness only on this set


# ---- samplers, forward ------------------------------------------------------------------------------------------------------
def _field(c):
    """what rodynrf.sampleXYZ reads of a field"""
    box = c["box"] if c.get("box") is not None else G.BOX
    return types.SimpleNamespace(near_far=[float(c["near"]), float(c["far"])], _aabb_host=[float(v) for v in np.asarray(box).reshape(-1)],
                                 _step_host=float(c.get("step", 0.0)), nSamples=c["S"])


def _sample(c):
    import rodynrf
    return rodynrf.sampleXYZ(_field(c), _cu(c["rays"]), c["S"], ray_type=c["kind"], is_train=False, jitter=_cu(c["jitter"]),
                             jitter_outer=_cu(c.get("jout")))


def _own_box_test(xyz, box):
    lo, hi = _cu(np.asarray(box[0], np.float32)), _cu(np.asarray(box[1], np.float32))
    return ~((lo > xyz) | (xyz > hi)).any(-1)


@pytest.mark.parametrize("kind", ["ndc", "contract", "world"])
def test_samplers_match_float64(kind):
    """xyz and z to the bound; `valid` EXACTLY the box test of the kernel's own xyz, and the float64 mask wherever the float64 point
    is farther from every face than its bound; points ON a face (exactly representable rays) are valid"""
    for tag, k in G.sampler_cases():
        if k["kind"] != kind:
            continue
        c = G.sampler_case(**k)
        ref = c["ref"]
        xyz, z, valid = _sample(c)
        _check(xyz, ref["xyz"], tag + " xyz")
        _check(z, ref["z"], tag + " z")
        assert valid.dtype == torch.bool
        if kind == "contract":
            assert bool(valid.all())
        else:
            assert torch.equal(valid, _own_box_test(xyz, c["box"])), f"{tag}: valid is not the box test of the returned points"
            clear = ref["clear"] > 0
            assert np.array_equal(valid.cpu().numpy()[clear], ref["valid"][clear]), f"{tag}: valid differs from the float64 mask"
    if kind == "contract":
        c = G.contract_exact_case()
        xyz, z, valid = _sample(c)
        assert np.array_equal(z.cpu().numpy()[:, :4].astype(np.float64), np.tile(c["z_inner"], (2, 1))), "dyadic inner midpoints are exact"
        assert np.array_equal(xyz.cpu().numpy()[:, :2].astype(np.float64), c["pts_inner"]), "dyadic points inside the unit cube are exact"
        return
    c = G.on_face_case(kind)
    if kind == "ndc":
        ref = G.sample_ndc_ref(c["rays"], c["S"], c["near"], c["far"], None, c["box"])
    else:
        ref = G.sample_world_ref(c["rays"], c["S"], c["near"], c["far"], c["step"], None, c["box"])
    xyz, z, valid = _sample(c)
    assert np.array_equal(xyz.cpu().numpy().astype(np.float64), ref["xyz"].v), f"on-face {kind}: the points are exactly representable"
    assert np.array_equal(valid.cpu().numpy(), c["expect"]), f"on-face {kind}: p == hi and p == lo are inside"
    if kind == "world":   # d_k == 0 on each axis in turn, rays from inside, rays whose entry lies beyond far
        for S in (1, 65):
            b = G.sample_world_bwd_case(S)
            cw = dict(kind="world", rays=b["rays"], S=S, near=b["near"], far=b["far"], step=0.0123, jitter=None, box=b["box"])
            ref = G.sample_world_ref(cw["rays"], S, cw["near"], cw["far"], cw["step"], None, cw["box"])
            xyz, z, valid = _sample(cw)
            _check(xyz, ref["xyz"], f"sample world rows S={S} xyz")
            _check(z, ref["z"], f"sample world rows S={S} z")
            assert torch.equal(valid, _own_box_test(xyz, cw["box"]))


# ---- sampler adjoints -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ndc", "contract"])
def test_sample_bwd_matches_float64(kind):
    """g_rays += onto a pre-fill; contract rows with samples on both sides of nrm = 1 and the arg-max on every axis and sign"""
    L = pkg()
    for S in G.SAMPLE_BWD_S:
        for N in (1, 3, 6):
            c = G.sample_bwd_case(kind, N, S)
            rays, z, g, gr = _cu(c["rays"]), _cu(c["z"]), _cu(c["g"]), _cu(c["pre"])
            L.check(L.lib.rdrf_sample_bwd(L.ptr(rays), L.ptr(z), N, S, L.RAY_TYPES[kind], L.ptr(g), L.ptr(gr), L.stream_of(gr)), "sample_bwd")
            _check(gr, c["ref"]["g_rays"], f"sample_bwd {kind} N={N} S={S}")


def _world_bwd(c):
    L = pkg()
    rays, z, g, gz, gr = _cu(c["rays"]), _cu(c["z"]), _cu(c["g"]), _cu(c["gz"]), _cu(c["pre"])
    ab = (C.c_float * 6)(*[float(v) for v in np.asarray(c["box"]).reshape(-1)])
    L.check(L.lib.rdrf_sample_world_bwd(L.ptr(rays), L.ptr(z), z.shape[0], z.shape[1], c["near"], c["far"], ab, L.ptr(g), L.ptr(gz), L.ptr(gr),
                                        L.stream_of(gr)), "sample_world_bwd")
    return gr


@pytest.mark.parametrize("S", G.SAMPLE_BWD_S)
def test_sample_world_bwd_matches_float64(S):
    """one ray per branch (G.WORLD_BWD_ROWS): t_min from each axis and slab side, raw below near / above far (nothing flows
    through t_min), raw == near exactly (the interval is closed: it flows), d_axis == 0 clamped and, with far = 1e7, selected
    (go gets the 1e-6 quotient, gd nothing); g_xyz and g_z each null in turn; g_rays pre-filled"""
    for m in ("both", "xyz", "z"):
        c = G.sample_world_bwd_case(S, m)
        _check(_world_bwd(c), c["ref"]["g_rays"], f"sample_world_bwd S={S} {m}")
    c = G.sample_world_bwd_zero_case(S)
    _check(_world_bwd(c), c["ref"]["g_rays"], f"sample_world_bwd S={S} d == 0 selected")


# ---- induced flow -----------------------------------------------------------------------------------------------------------
def _flow_gpu(c, g_flow=True, g_disp=True, null=None):
    L = pkg()
    N, S = c["w"].shape
    rt = L.RAY_TYPES["contract" if c["contract"] else "ndc"]
    f, c2w, w, pts, p2d, rays = (_cu(np.asarray(c[k]).reshape(1) if k == "focal" else c[k]) for k in ("focal", "c2w", "w", "pts", "p2d", "rays"))
    flow, disp = torch.empty(N, 2, device="cuda"), torch.empty(N, device="cuda")
    L.check(L.lib.rdrf_induce_flow_fwd(c["H"], c["W"], L.ptr(f), L.ptr(c2w), L.ptr(w), L.ptr(pts), L.ptr(p2d), L.ptr(rays), N, S, rt,
                                       L.ptr(flow), L.ptr(disp), L.stream_of(w)), "induce_flow_fwd")
    outs = {k: (None if k == null else _cu(c["pre"][k])) for k in G.FLOW_OUTS}
    gfl, gdi = (_cu(c["g_flow"]) if g_flow else None), (_cu(c["g_disp"]) if g_disp else None)
    L.check(L.lib.rdrf_induce_flow_bwd(c["H"], c["W"], L.ptr(f), L.ptr(c2w), L.ptr(w), L.ptr(pts), L.ptr(rays), N, S, rt, L.ptr(gfl), L.ptr(gdi),
                                       L.ptr(outs["g_weights"]), L.ptr(outs["g_pts"]), L.ptr(outs["g_rays"]), L.ptr(outs["g_c2w"]),
                                       L.ptr(outs["g_focal"]), L.stream_of(w)), "induce_flow_bwd")
    return dict(outs, flow=flow, disp=disp)


def _flow_ref(c, g_flow=True, g_disp=True):
    return G.flow_ref(c["H"], c["W"], c["focal"], c["c2w"], c["w"], c["pts"], c["p2d"], c["rays"], c["contract"],
                      c["g_flow"] if g_flow else None, c["g_disp"] if g_disp else None, c["pre"])


FLOW_CASES = G.flow_cases()


@pytest.mark.parametrize("tag,k", FLOW_CASES, ids=[t for t, _ in FLOW_CASES])
def test_induce_flow_and_adjoint_match_float64(tag, k):
    """flow, disparity and all five gradients ACCUMULATED onto pre-fills, g_focal against the float64 sum on every case, no ray
    masked; g_flow / g_disp null in turn; each output pointer null in turn; the clamp of P.z passes exactly nothing"""
    c = G.flow_case(**k)
    for gfl, gdi, null in [(True, True, None), (False, True, None), (True, False, None)] + [(True, True, n) for n in G.FLOW_OUTS]:
        ref = c["ref"] if (gfl and gdi) else _flow_ref(c, gfl, gdi)
        got = _flow_gpu(c, gfl, gdi, null)
        sub = f"{tag} g_flow={gfl} g_disp={gdi} null={null}"
        for name in ("flow", "disp") + G.FLOW_OUTS:
            if name != null:
                _check(got[name], ref[name], f"{sub} {name}")
        if not c["contract"] and null != "g_pts":
            cl = torch.from_numpy(ref["clamped"])
            assert bool(cl.any()) or k["N"] < 7
            assert torch.equal(got["g_pts"].cpu()[cl][:, :, 2], torch.from_numpy(c["pre"]["g_pts"])[cl][:, :, 2]), \
                f"{sub}: gP[2] must be exactly 0 where P.z is clamped"


@pytest.mark.parametrize("contract", [False, True])
def test_induce_flow_near_singular_set(contract):
    c = G.flow_case(contract, 128, 13, singular=True)
    ref = c["ref"]
    got = _flow_gpu(c)
    for name in ("flow", "disp", "g_weights", "g_pts", "g_rays", "g_c2w"):
        _check(got[name], ref[name], f"flow near-singular {'contract' if contract else 'ndc'} {name}", ref[name].r > G.RHO_LIMIT)
    assert bool(torch.isfinite(got["g_focal"]).all())   # the sum over every ray, the over-limit ones included: finiteness only
