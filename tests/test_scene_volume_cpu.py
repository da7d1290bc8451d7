"""CPU-side checks of the whole-scene volumes (csrc/rdrf_scene_alpha.hip, alpha.scene_alpha_volume): the float64 reference
of tests/_scene_prim.py against the oracle's compositor and against the reference-generated goldens, the kernel's arithmetic
restated in fp32 against the bounds the GPU tests use, planted defects against the same bounds, and the argument refusals of
the Python layer that need no device.

The `+ 1e-10` defect: in fp32 the term is below the resolution of alpha (1e-10 < 2^-24 / 500; 1 - (pq + 1e-10) rounds to
1 - pq or its neighbour), so no bound of k 2^-24 can see it -- it is planted in the float64 evaluation instead and falls
outside the 1e-12 at which the reference is held to the oracle's factor."""
import types

import numpy as np
import pytest
import torch

import _scene_prim as P
from _util import CASES, load_case, pkg, record_margin

LENGTH = 0.08


def _oracle_two_sample(ss, sd, b, length):
    """the oracle's raw2outputs on two-sample rays whose first sample is the entry (dists[0] = length) and whose second is an
    opaque dynamic one (weight 1): weights_full[:, 1] = T_full[:, 1], the first sample's factor; the first sample's colours
    (1, 0, 0) dynamic and (0, 1, 0) static leave w_d and w_s in the first two channels of rgb_map_full"""
    from oracle import rodynrf_oracle as O
    n = len(ss)
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))
    col = lambda v: torch.stack([t(v), torch.full((n,), 1e9, dtype=torch.float64)], -1)
    sigma_s, sigma_d = torch.stack([t(ss), torch.zeros(n, dtype=torch.float64)], -1), col(sd)
    blending = torch.stack([t(b), torch.ones(n, dtype=torch.float64)], -1)
    dists = torch.tensor([float(length), 1.0], dtype=torch.float64).repeat(n, 1)
    rgb_d, rgb_s = torch.zeros(n, 2, 3, dtype=torch.float64), torch.zeros(n, 2, 3, dtype=torch.float64)
    rgb_d[:, 0, 0], rgb_s[:, 0, 1] = 1.0, 1.0
    rays = torch.zeros(n, 6, dtype=torch.float64)
    out = O.raw2outputs(rgb_s, sigma_s, rgb_d, sigma_d, dists, blending, torch.zeros(n, 2, dtype=torch.float64), rays)
    return out[3][:, 1].numpy(), out[0][:, 0].numpy(), out[0][:, 1].numpy()


def test_reference_matches_the_oracle_factor():
    ss, sd, b = P.ingredients(4000, 1, LENGTH)
    T1, wd, ws = _oracle_two_sample(ss, sd, b, np.float32(LENGTH))
    alpha, owner, den = P.compose(ss, sd, b, np.float32(LENGTH))
    err = float(np.abs(alpha - (1.0 - (T1 - 1e-10))).max())
    record_margin("reference alpha vs oracle T_full", err / 1e-12)
    assert err <= 1e-12, err
    assert float(np.abs(den - (wd + ws)).max()) <= 1e-12
    # the owner over its condition scale, as the bounds treat it: owner (w_d + w_s) against the oracle's w_d (a quotient of two
    # numbers of 1e-5 moves by 1e-16 / 1e-5 with the last bit of a library's exp)
    nz = (wd + ws) > 0
    assert float(np.abs(owner * (wd + ws) - wd).max()) <= 1e-12 and bool((owner[~nz] == 0).all())    # the planted `+ 1e-10` leaves that tolerance
    kept = P.compose(ss, sd, b, np.float32(LENGTH), defect="keep_eps")[0]
    assert float(np.abs(kept - (1.0 - (T1 - 1e-10))).min()) > 50e-12


@pytest.mark.parametrize("case", CASES)
def test_reference_matches_the_goldens(case):
    """the goldens hold the reference's per-sample sigma of both fields, blending and dists and its weights_full =
    (w_d + w_s) T_full with T_full the running product of 1 - alpha + 1e-10: rebuilt from this file's reference per sample
    (length = that sample's dists) and compared with what the reference's fp32 compositor stored.  Each of its factors carries
    a few ulp and the product of s of them s times that: (6 s + 8) 2^-24, absolute, weights being at most 1"""
    g = load_case(case)[0]
    ss, sd, b, dists = g["fs.sigma"], g["fd.sigma"], g["fd.blending"], g["fd.dists"]
    S = ss.shape[1]
    alpha, _, den = P.compose(ss, sd, b, dists)
    T = np.cumprod(np.concatenate([np.ones_like(alpha[:, :1]), 1.0 - alpha + 1e-10], -1), -1)[:, :-1]
    err = np.abs(den * T - g["ce.weights_full"])
    bound = (6.0 * np.arange(S) + 8.0) * P.U24
    record_margin(f"{case} weights_full rebuilt from the reference", float((err / bound).max()))
    assert bool((err <= bound).all()), float((err / bound).max())
    assert float(np.abs((den * T).sum(-1) - g["ce.acc_map_full"]).max()) <= (6.0 * S + 8.0) * P.U24 * 4
    assert float(g["ce.acc_map_full"].max()) > 0.05 and float(g["ce.weights_full"].max()) > 1e-3   # the case is not empty


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_fp32_evaluation_lies_inside_the_bounds(seed):
    ss, sd, b = P.ingredients(200000, seed, LENGTH)
    a32, o32, _ = P.compose(ss, sd, b, np.float32(LENGTH), dtype=np.float32)
    wa, wo, ok = P.check(a32, o32, ss, sd, b, np.float32(LENGTH))
    record_margin("fp32 restatement alpha", wa)
    record_margin("fp32 restatement owner", wo)
    assert ok and wa <= 1.0 and wo <= 1.0, (wa, wo, ok)
    assert wa > 0.05   # the bound is not orders of magnitude loose
    # the edge entries are there and exact
    both = (ss == 0) & (sd == 0)
    assert both.sum() > 100 and bool((a32[both] == 0).all()) and bool((o32[both] == 0).all())
    sat = (sd * np.float32(LENGTH) > 40) & (b == 1)
    assert sat.sum() > 10 and bool((a32[sat] == 1).all()) and bool((o32[sat] == 1).all())


@pytest.mark.parametrize("defect", ["swap_b", "a_s_from_sigma_d"])
def test_planted_defects_fall_outside_the_bounds(defect):
    ss, sd, b = P.ingredients(200000, 3, LENGTH)
    a32, o32, _ = P.compose(ss, sd, b, np.float32(LENGTH), dtype=np.float32, defect=defect)
    wa, wo, _ = P.check(a32, o32, ss, sd, b, np.float32(LENGTH))
    assert wa > 1000.0 and wo > 1000.0, (defect, wa, wo)


def test_a_nan_ingredient_is_a_nan_in_that_entry_only():
    ss, sd, b = P.ingredients(3000, 4, LENGTH)
    for k, arr in enumerate((ss, sd, b)):
        arr[k::7] = np.nan
    a32, o32, _ = P.compose(ss, sd, b, np.float32(LENGTH), dtype=np.float32)
    nan = np.isnan(ss) | np.isnan(sd) | np.isnan(b)
    assert np.array_equal(np.isnan(a32), nan) and np.array_equal(np.isnan(o32), nan)
    assert P.check(a32, o32, ss, sd, b, np.float32(LENGTH))[2]


def test_python_layer_refuses_bad_arguments_by_name():
    import rodynrf
    A = pkg("alpha")
    st = types.SimpleNamespace(DYNAMIC=False, aabb=torch.zeros(2, 3), alphaMask=None)
    dy = types.SimpleNamespace(DYNAMIC=True, aabb=torch.zeros(2, 3), alphaMask=None, _step_host=0.1)
    far = types.SimpleNamespace(DYNAMIC=True, aabb=torch.zeros(2, 3, device="meta"), alphaMask=None, _step_host=0.1)
    xyz = torch.zeros(4, 3)
    with pytest.raises(rodynrf.RdrfError, match="want"):
        rodynrf.scene_alpha_volume(st, dy, xyz, [0.0], want=("alpha", "rgb"))
    with pytest.raises(rodynrf.RdrfError, match="want"):
        rodynrf.scene_alpha_volume(st, dy, xyz, [0.0], want=())
    with pytest.raises(rodynrf.RdrfError, match="tensorf_static is on cpu and tensorf on meta"):
        rodynrf.scene_alpha_volume(st, far, xyz, [0.0])
    with pytest.raises(rodynrf.RdrfError, match="tensorf_static must be the static field"):
        rodynrf.scene_alpha_volume(dy, dy, xyz, [0.0])
    with pytest.raises(rodynrf.RdrfError, match="tensorf must be the dynamic field"):
        rodynrf.scene_dense_alpha(st, st)
    with pytest.raises(rodynrf.RdrfError, match="masks"):
        rodynrf.scene_alpha_volume(st, dy, xyz, [0.0], masks="both")
    with pytest.raises(rodynrf.RdrfError, match="xyz"):
        rodynrf.scene_alpha_volume(st, dy, torch.zeros(4, 2), [0.0])
    with pytest.raises(rodynrf.RdrfError, match="CPU tensor"):   # no fallback: the points must be on the device
        rodynrf.scene_alpha_volume(st, dy, xyz, [0.0])
    for fn in (rodynrf.scene_mesh, rodynrf.colored_scene_mesh):
        with pytest.raises(rodynrf.RdrfError, match="pass t"):
            fn(st, dy)
    with pytest.raises(rodynrf.RdrfError, match="pass t"):
        rodynrf.scene_vertex_colors(st, dy, xyz)
    with pytest.raises(rodynrf.RdrfError, match="pass t"):
        rodynrf.export_mesh(dy, "unused.ply", static=st)
    with pytest.raises(rodynrf.RdrfError, match="simplify"):
        rodynrf.scene_mesh(st, dy, 0.0, simplify=0)
    with pytest.raises(rodynrf.RdrfError, match="space"):
        rodynrf.scene_mesh_sequence(st, dy, [0.0], space="camera")
    with pytest.raises(rodynrf.RdrfError, match="both fields must be on one device"):
        rodynrf.scene_mesh_sequence(st, far, [0.0])
    assert A.SCENE_OUTPUTS == P.ORDER


def test_c_entry_point_refuses_before_any_device_work():
    """M == 0 is a no-op; T < 1, every output null, M * T beyond 2^31 - 1 and a short workspace are refused on the host (null
    device pointers throughout: a launch would not survive them)"""
    import ctypes as C
    L = pkg()
    PS, PD, cs, cd = L.RdrfStaticParams(), L.RdrfDynamicParams(), L.RdrfFieldCfg(), L.RdrfFieldCfg()
    one = C.c_void_p(256)   # a non-null pointer that is never followed

    def call(M, T, outs, ws_bytes):
        return L.lib.rdrf_scene_alpha(C.byref(PS), C.byref(cs), C.byref(PD), C.byref(cd), one, M, one, T, 0.1, None, None, *outs,
                                      one, ws_bytes, None)

    big = L.lib.rdrf_scene_alpha_ws_bytes(1 << 20, 4096)
    none, alpha = [None] * 5, [one] + [None] * 4
    assert call(0, 0, none, 0) == 0
    assert call(5, 0, alpha, big) == -1 and b"T" in L.lib.rdrf_last_error()
    assert call(-1, 1, alpha, big) == -1
    assert call(5, 1, none, big) == -1 and b"every output is null" in L.lib.rdrf_last_error()
    assert call(1 << 20, 4096, alpha, big) == -1 and b"M * T" in L.lib.rdrf_last_error()
    assert L.lib.rdrf_scene_alpha_ws_bytes(100, 3) > L.lib.rdrf_scene_alpha_ws_bytes(0, 3) > 0
    for i in range(5):   # each output alone passes the "every output is null" check and reaches the next refusal
        outs = [one if j == i else None for j in range(5)]
        assert call(5, 1, outs, 0) != 0 and b"every output is null" not in L.lib.rdrf_last_error()
