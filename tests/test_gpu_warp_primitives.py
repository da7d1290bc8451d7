"""The data gradients of the warp MLP's flat tile (rdrf_selftest_warp_bwd: k_dyn_warp_bwd_dw) and of the scene-flow backward
(rdrf_scene_flow_bwd: k_scene_flow_bwd_dw) against the float64 references of tests/_warp_prim.py, on rows the test supplies, through
the harnesses of test_gpu_warp_dw_fused.py / test_gpu_scene_flow_fused.py with the box a parameter.  g_xyz / g_pts, dtout and dtp sit
between NaN-poisoned guard bands of 64 floats; the outputs that are added into are pre-filled with small integers that join the
reference.  The feature-mode warp tile and the wave-per-ray warp tile are not reachable through these entry points (_warp_prim.py).

  exact   integer inputs on the box [-2, 2] x [-1, 1] x [-4, 4] (inv = 0.5, 1, 0.25): g_xyz, the dd rows, d(tout) per ray and g_pts
          bit for bit, at the tile edge, with a ray spanning tiles, with fewer tiles than waves and with two waves in a workgroup; with
          and without g_xyz_prime; with g_xyz absent (nothing else changes, its buffer and bands stay as they were); the scene flow
          with either or both upstream gradients, and on its own box onto zeros, where g_pts = fl32(e inv32).
  dense   normal rows (the X0 rows independent normals, and the real sin / cos of a drawn xn) and gate_edges (H rows from {+-0,
          +-2^-126, +-1}) on the box [-1.5, 1.5] x [-1.67, 1.67] x [-1, 1]: every element within its bound k 2^-24 cond.
  bands   after every call the guard bands are intact and the dtout / dtp slots the kernel does not own keep their fill.
  tools   the tools build, one child per setting of RDRF_WARP_FUSED / RDRF_SF_FUSED: the dense outputs of the fused and of the
          two-kernel path are each held to the same bounds.
Why each assertion is there: the mutation table of test_warp_primitives_cpu.py."""
import numpy as np
import pytest

import _heads_prim as HP
import _warp_prim as Q
from _twin import CHILD, run_twin, tools_lib
from _util import pkg, record_margin

f32, f64 = np.float32, np.float64
_REF = {}


def _wf():
    import test_gpu_warp_dw_fused as WF
    return WF


def _sf():
    import test_gpu_scene_flow_fused as SF
    return SF


def _rows3(sm):
    """the small-layer dz rows [T][3][32] -> [T 32][3]"""
    return sm.transpose(0, 2, 1).reshape(sm.shape[0] * 32, 3)


# ---- warp --------------------------------------------------------------------------------------------------------------------------
def warp_run(c, gx=True, H=None):
    out = (H or _wf()._harness()).run(c, gx=gx, gp=c["gp"] is not None, box=c["box"])
    assert all(out["guards"].values()), f"guard bands written: {out['guards']}"
    return out


def owned_slots(N, S):
    """which dtout rows [N] and dtp records [T][2] the kernel writes (brute force: _heads_prim.tile_records)"""
    dtout, dtp = HP.tile_records(np.zeros((N * S, 30)), N, S)
    return ~np.isnan(dtout[:, 0]), ~np.isnan(dtp[:, :, 0])


def check_slots(c, out):
    """slots the kernel does not own keep their fill; an owned record's columns 30, 31 (no column of layer3 behind them) are 0"""
    WF = _wf()
    own_t, own_p = owned_slots(c["N"], c["S"])
    assert (out["dtout"][~own_t] == WF.DT_FILL).all() and (out["dtp"][~own_p] == WF.DT_FILL).all(), "a slot the kernel does not own was written"
    assert not out["dtout"][own_t][:, 30:].any() and not out["dtp"][own_p][:, 30:].any()


def warp_case_ref(kind, N, S, **kw):
    key = ("warp", kind, N, S, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _REF:
        lay = Q.warp_layout(pkg())
        c = Q.warp_case(lay, kind, N, S, **kw)
        _REF[key] = (c, Q.warp_reference(c, lay))
    return _REF[key]


def check_warp_exact(c, ref, out, tag):
    if out["g_xyz"] is not None:
        assert np.array_equal(out["g_xyz"].astype(f64), ref["g_xyz"][0]), f"{tag}: g_xyz differs from the exact sums"
    else:
        assert np.array_equal(out["g_xyz_unused"].view(np.uint32), out["pre_g"].view(np.uint32)), f"{tag}: the absent g_xyz was written"
    assert np.array_equal(_rows3(out["sm"]).astype(f64), ref["dd"][0]), f"{tag}: the dd rows differ"
    assert np.array_equal(_wf().ray_dtout(c, out["dtout"], out["dtp"]), ref["dtout"][0]), f"{tag}: d(tout) differs"
    check_slots(c, out)


@pytest.mark.gpu
@pytest.mark.parametrize("N,S", Q.WARP_EXACT)
def test_warp_exact(N, S):
    for gp in (True, False):
        c, ref = warp_case_ref("exact", N, S, seed=int(gp), gp=gp)
        a = warp_run(c)
        check_warp_exact(c, ref, a, f"warp exact {N}x{S} gp {int(gp)}")
        b = warp_run(c, gx=False)
        check_warp_exact(c, ref, b, f"warp exact {N}x{S} gp {int(gp)} no g_xyz")
        for k in ("sm", "dtout", "dtp"):
            assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), f"{k} changes when g_xyz is absent"


WARP_DENSE_CASES = [(kind, enc, N, S) for N, S in Q.WARP_DENSE for kind, enc in (("dense", "normal"), ("dense", "sincos"), ("gate_edges", "normal"))]


def warp_ratios(c, ref, out):
    return {"g_xyz": Q.ratio(out["g_xyz"], *ref["g_xyz"]), "dd": Q.ratio(_rows3(out["sm"]), *ref["dd"]),
            "dtout": Q.ratio(_wf().ray_dtout(c, out["dtout"], out["dtp"]), *ref["dtout"])}


def check_warp_dense(c, ref, out, tag, record=True):
    rat = warp_ratios(c, ref, out)
    for k, v in rat.items():
        print(f"{tag} {k}: error / bound = {v:.4f}")
        if record:
            record_margin(f"{tag} {k}", v)
    assert all(v <= 1.0 for v in rat.values()), (tag, rat)
    check_slots(c, out)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,enc,N,S", WARP_DENSE_CASES)
def test_warp_dense(kind, enc, N, S):
    for gp in (True, False):
        c, ref = warp_case_ref(kind, N, S, box=Q.BOX_ODD, enc=enc, gp=gp)
        check_warp_dense(c, ref, warp_run(c), f"warp {kind} {enc} {N}x{S} gp {int(gp)}")


# ---- scene flow ----------------------------------------------------------------------------------------------------------------------
def sf_run(c, H=None):
    H = H or _sf()._harness()
    g = H.run(c["n"], c["rows"], c["W"], c["gf"], c["gb"], pts=True, prefill=False, box=c["box"], pts_fill=c["pre"])[2]
    assert H.guards_intact, "the guard bands of g_pts were written"
    return g.reshape(c["n"], 3)


def sf_case_ref(kind, n, **kw):
    key = ("sf", kind, n, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _REF:
        lay = Q.sf_layout(pkg())
        c = Q.sf_case(lay, kind, n, **kw)
        _REF[key] = (c, Q.sf_reference(c, lay))
    return _REF[key]


LIVE = [(True, True), (True, False), (False, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("n", Q.SF_EXACT)
def test_scene_flow_exact(n):
    for seed, (gf, gb) in enumerate(LIVE):
        c, ref = sf_case_ref("exact", n, seed=seed, gf=gf, gb=gb)
        assert np.array_equal(sf_run(c).astype(f64), ref["g_pts"][0]), f"scene flow exact {n} f {gf} b {gb}: g_pts differs from the exact sums"
        c, ref = sf_case_ref("exact", n, seed=seed, gf=gf, gb=gb, box=Q.BOX_ODD, prefill=False)
        want = ref["e"][0].astype(f32) * Q.box_inv(c["box"])[None, :] + f32(0.0)
        assert np.array_equal(sf_run(c).view(np.uint32), want.view(np.uint32)), f"scene flow exact {n} f {gf} b {gb}: g_pts is not fl32(e inv32)"


SF_DENSE_CASES = [("dense", "normal"), ("dense", "sincos"), ("gate_edges", "normal")]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,enc", SF_DENSE_CASES)
def test_scene_flow_dense(kind, enc):
    for gf, gb in LIVE:
        c, ref = sf_case_ref(kind, Q.SF_DENSE, box=Q.BOX_ODD, enc=enc, gf=gf, gb=gb)
        v = Q.ratio(sf_run(c), *ref["g_pts"])
        tag = f"scene flow {kind} {enc} f {int(gf)} b {int(gb)} g_pts"
        print(f"{tag}: error / bound = {v:.4f}")
        record_margin(tag, v)
        assert v <= 1.0, (tag, v)


# ---- the tools build: both partners against the same bounds ---------------------------------------------------------------------------
def warp_tools_case():
    """the dense outputs of whichever path RDRF_WARP_FUSED selects (tests/_det_child.py case)"""
    H = _wf().Harness()
    res = {}
    for i, (kind, enc, N, S) in enumerate(WARP_DENSE_CASES):
        c, _ = warp_case_ref(kind, N, S, box=Q.BOX_ODD, enc=enc, gp=True)
        out = warp_run(c, H=H)
        for k in ("g_xyz", "sm", "dtout", "dtp"):
            res[f"{i}.{k}"] = out[k]
    return res


def sf_tools_case():
    """the dense g_pts of whichever path RDRF_SF_FUSED selects"""
    H = _sf().Harness()
    return {str(i): sf_run(sf_case_ref(kind, Q.SF_DENSE, box=Q.BOX_ODD, enc=enc, gf=True, gb=True)[0], H=H) for i, (kind, enc) in enumerate(SF_DENSE_CASES)}


def _child(tmp_path, func, env):
    res = run_twin(tmp_path, [CHILD, "case", "test_gpu_warp_primitives", func], lib=tools_lib(), extra_env=env)
    return {k: v.numpy() for k, v in res.items()}


@pytest.mark.gpu
def test_tools_build_warp_partners(tmp_path):
    for fused in ("1", "0"):   # one child after the other
        got = _child(tmp_path, "warp_tools_case", {"RDRF_WARP_FUSED": fused})
        for i, (kind, enc, N, S) in enumerate(WARP_DENSE_CASES):
            c, ref = warp_case_ref(kind, N, S, box=Q.BOX_ODD, enc=enc, gp=True)
            check_warp_dense(c, ref, {k: got[f"{i}.{k}"] for k in ("g_xyz", "sm", "dtout", "dtp")}, f"tools fused {fused} warp {kind} {enc} {N}x{S}")


@pytest.mark.gpu
def test_tools_build_scene_flow_partners(tmp_path):
    for fused in ("1", "0"):
        got = _child(tmp_path, "sf_tools_case", {"RDRF_SF_FUSED": fused})
        for i, (kind, enc) in enumerate(SF_DENSE_CASES):
            _, ref = sf_case_ref(kind, Q.SF_DENSE, box=Q.BOX_ODD, enc=enc, gf=True, gb=True)
            v = Q.ratio(got[str(i)], *ref["g_pts"])
            tag = f"tools fused {fused} scene flow {kind} {enc} g_pts"
            print(f"{tag}: error / bound = {v:.4f}")
            record_margin(tag, v)
            assert v <= 1.0, (tag, v)
