"""The forward VM gather and the positional encodings on their own (rdrf_selftest_gather / rdrf_selftest_encodings: the device
functions of the forward kernels, unchanged, one wave per 32 points) against the numpy references of tests/_gather_prim.py, and the
same batches through the public per-point entry points.

Exact class: 2^k + 1 grids, dyadic coordinates, distinct integers: every term of every output is a multiple of 2^-q with
sum |terms| 2^q < 2^24 (asserted by the reference, tests/test_gather_primitives_cpu.py), so neither the order of the sums nor an
fma can change a bit: array_equal.  Dense class: normal data on grids whose L - 1 is no multiple of the stride and on axes so short
that a level collapses to one texel, at every edge coordinate; with u = 2^-24 and the reference exact on the same float32 weights,
|err| <= 8 u P Lm per feature (one rounding for the weight product, four for the bilinear sum, two for the line, one for the
product; an fma only lowers it) and |err| <= 32 u sum_f P_f Lm_f for the static density sum (24 more additions).  Encodings:
the bound of test_abi_cpu.py::test_sincos_pe_formula on the fast path, 4 ulp of 1 (OpenCL's sin / cos accuracy, |result| <= 1) for
every lane of a wave that holds a wild lane.  The ratios of one RDRF_MARGINS run are in profiles/gather_margins.txt."""
import ctypes as C

import numpy as np
import pytest
import torch

import _gather_prim as G
from _scatter_prim import plane_dims
from _util import FWD_ELEM, elementwise_excess, pkg, record_margin

pytestmark = pytest.mark.gpu

GUARD = -7.0
f32 = np.float32


class DevSets:
    """factor sets on the device as an RdrfVM array; order "W": planes stored [H][W][C], "H": [W][H][C]"""

    def __init__(self, kind, sets, grid, order="W"):
        L = pkg()
        self.kind, self.n = kind, len(sets)
        self.vm = (L.RdrfVM * self.n)()
        self.keep = []
        for i, (planes, lines) in enumerate(sets):
            for p, (W, H, Ln) in enumerate(plane_dims(grid)):
                Cn = planes[p].shape[2]
                phys = planes[p] if order == "W" else np.transpose(planes[p], (1, 0, 2))
                pl = torch.from_numpy(np.ascontiguousarray(phys)).float().cuda()
                ln = torch.from_numpy(np.ascontiguousarray(lines[p])).float().cuda()
                self.keep += [pl, ln]
                vm = self.vm[i]
                vm.plane[p], vm.line[p], vm.C[p], vm.H[p], vm.W[p], vm.L[p] = pl.data_ptr(), ln.data_ptr(), Cn, H, W, Ln
                vm.sH[p], vm.sW[p] = (W * Cn, Cn) if order == "W" else (Cn, H * Cn)

    def run(self, xn):
        """-> [nsets][M][F] float64; the rows behind M keep their fill"""
        L = pkg()
        xn = np.ascontiguousarray(xn, dtype=f32).reshape(-1, 3)
        M = xn.shape[0]
        F = 1 if self.kind == "STATIC_DENSITY" else G.nfeat(self.kind)
        x = torch.from_numpy(xn).cuda()
        out = torch.full((self.n * M * F + 64,), GUARD, device="cuda")
        L.check(L.lib.rdrf_selftest_gather(L.SCATTER_KINDS[self.kind], C.cast(self.vm, C.c_void_p), self.n, L.ptr(x), M, L.ptr(out),
                                           L.stream_of(out)), f"rdrf_selftest_gather {self.kind}")
        got = out.cpu().double().numpy()
        assert (got[self.n * M * F:] == GUARD).all(), "floats behind the last point were written"
        return got[: self.n * M * F].reshape(self.n, M, F)


def _want_exact(kind, feat):
    return feat.sum(-1, keepdims=True) if kind == "STATIC_DENSITY" else feat


def _dense_ratio(kind, got, ref):
    """max |err| / bound; where the bound is 0 every tap weight or value is 0 and the result must be 0.0"""
    feat, P, Lm = ref
    if kind == "STATIC_DENSITY":
        want, mag = G.static_density(feat, P, Lm)
        want, bound = want[:, None], 32 * G.U * mag[:, None]
    else:
        want, bound = feat, 8 * G.U * P * Lm
    err = np.abs(got - want)
    assert np.isfinite(got).all()
    assert (err[bound == 0] == 0).all(), "a feature without any live tap must be exactly 0.0"
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


# ---- the primitives ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("grid", G.EXACT_GRIDS, ids=str)
def test_gather_exact_cases_bit_for_bit(kind, grid):
    c = G.exact_case(kind, grid)
    rng = np.random.default_rng(11)
    for order in ("W", "H"):
        dev = DevSets(kind, c["sets"], grid, order)
        for M in G.MS if order == "W" else (33, 97):
            perm = rng.permutation(len(c["xn"]))[:M]        # shuffled: the edge points change lane and half-wave
            got = dev.run(c["xn"][perm])
            for s in range(dev.n):
                want = _want_exact(kind, c["ref"][s][perm])
                bad = np.nonzero(got[s] != want)
                assert len(bad[0]) == 0, (f"{kind} {grid} order {order} M={M} set {s}: {len(bad[0])} features differ, first at point "
                                          f"{bad[0][0]} (xn {c['xn'][perm][bad[0][0]]}) feature {bad[1][0]}: {got[s][bad[0][0], bad[1][0]]} != "
                                          f"{want[bad[0][0], bad[1][0]]}")


@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("grid", G.DENSE_GRIDS, ids=str)
def test_gather_dense_cases_within_derived_bounds(kind, grid):
    c = G.dense_case(kind, grid)
    dev = DevSets(kind, c["sets"], grid)
    worst = 0.0
    for b in G.batches(len(c["xn"])):
        got = dev.run(c["xn"][b])
        for s in range(dev.n):
            worst = max(worst, _dense_ratio(kind, got[s], tuple(r[b] for r in c["ref"][s])))
    record_margin(f"gather {kind} {grid}", worst)
    assert worst <= 1.0, f"{kind} {grid}: |err| is {worst:.3f} x the bound"


@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("grid", ((6, 7, 11), (2, 3, 5)), ids=str)
def test_gather_non_finite_points_are_zero_and_leave_their_neighbours_alone(kind, grid):
    """zero padding for NaN / +-inf in one, two or three axes (every address of axis_tap is clamped, fmed3f before the conversion
    and min(max()) behind it, whatever the coordinate): exactly 0.0, and the other points of the tile keep their bits"""
    c = G.dense_case(kind, grid)
    rng = np.random.default_rng(23)
    M = 65
    base = rng.uniform(-1.0, 1.0, (M, 3)).astype(f32)
    slots = rng.permutation(M)[: len(G.NONFINITE)]
    mixed = base.copy()
    mixed[slots] = np.asarray(G.NONFINITE, dtype=f32)
    dev = DevSets(kind, c["sets"], grid)
    clean, got = dev.run(base), dev.run(mixed)
    others = np.setdiff1d(np.arange(M), slots)
    assert (got[:, slots] == 0.0).all(), "a non-finite coordinate must give exactly 0.0"
    assert np.array_equal(got[:, others], clean[:, others])
    assert (clean[:, others] != 0.0).mean() > 0.9


# ---- the public entry points -------------------------------------------------------------------------------------------------
AABB = [[-1.5, -1.67, -1.0], [1.5, 1.67, 1.0]]
KW = dict(density_n_comp=[16, 4, 4], appearance_n_comp=[48, 12, 12], app_dim=27, alphaMask_thres=1e-4, distance_scale=25, pos_pe=6,
          view_pe=0, featureC=128, step_ratio=2.0, near_far=[0.0, 1.0], density_shift=-10.0, fea2denseAct="relu")


def _load_set(field, prefix, planes, lines):
    with torch.no_grad():
        for p in range(3):
            getattr(field, prefix + "_plane")[p].copy_(torch.from_numpy(planes[p]).float().permute(2, 0, 1)[None])
            getattr(field, prefix + "_line")[p].copy_(torch.from_numpy(lines[p]).float().permute(1, 0)[None, :, :, None])
    field.invalidate_packed()


def _static_field(grid, density, app):
    import rodynrf
    st = rodynrf.TensorVMSplit(torch.tensor(AABB), list(grid), 12, "cuda", shadingMode="MLP_Fea", fea_pe=2, **KW)
    _load_set(st, "density", *density)
    _load_set(st, "app", *app)
    return st


def _one_hot_app(st, xn, nfeat):
    """compute_appfeature with one-hot basis_mat rows: selection k passes components 27 k .. 27 k + 26 through the fp32 MFMA"""
    out = np.zeros((len(xn), nfeat))
    x = torch.from_numpy(np.ascontiguousarray(xn)).cuda()
    for k in range((nfeat + 26) // 27):
        n = min(27, nfeat - 27 * k)
        w = torch.zeros(27, nfeat)
        w[torch.arange(n), 27 * k + torch.arange(n)] = 1.0
        with torch.no_grad():
            st.basis_mat.weight.copy_(w)
        st.invalidate_packed()
        with torch.no_grad():
            out[:, 27 * k: 27 * k + n] = st.compute_appfeature(x).cpu().double().numpy()[:, :n]
    return out


@pytest.mark.parametrize("grid", G.EXACT_GRIDS, ids=str)
def test_static_feature_entry_points_exact_cases(grid):
    """rdrf_static_features_fwd on the exact batches: the density feature and, through one-hot basis rows (three selections cover the
    72 components; a one-hot selection passes the fp32 MFMA exactly), the gathered appearance components, bit for bit"""
    cd, ca = G.exact_case("STATIC_DENSITY", grid), G.exact_case("STATIC_APP", grid)
    st = _static_field(grid, cd["sets"][0], ca["sets"][0])
    with torch.no_grad():
        dens = st.compute_densityfeature(torch.from_numpy(cd["xn"]).cuda()).cpu().double().numpy()
    assert np.array_equal(dens, cd["ref"][0].sum(-1))
    assert np.array_equal(_one_hot_app(st, ca["xn"], 72), ca["ref"][0])


@pytest.mark.parametrize("grid", G.DENSE_GRIDS, ids=str)
def test_static_feature_entry_points_dense_cases(grid):
    cd, ca = G.dense_case("STATIC_DENSITY", grid), G.dense_case("STATIC_APP", grid)
    st = _static_field(grid, cd["sets"][0], ca["sets"][0])
    with torch.no_grad():
        dens = st.compute_densityfeature(torch.from_numpy(cd["xn"]).cuda()).cpu().double().numpy()
    r = _dense_ratio("STATIC_DENSITY", dens[:, None], cd["ref"][0])
    record_margin(f"static_features_fwd density {grid}", r)
    assert r <= 1.0, f"density feature {grid}: |err| is {r:.3f} x the 32 u bound"
    r = _dense_ratio("STATIC_APP", _one_hot_app(st, ca["xn"], 72), ca["ref"][0])
    record_margin(f"static_features_fwd app one-hot {grid}", r)
    assert r <= 1.0, f"appearance components {grid}: |err| is {r:.3f} x the 8 u bound"


def _round_trip(xn, aabb):
    """norm_c(unnorm_c(xn) + 0) of csrc/rdrf_common.hpp in float32, one rounding per operation (contraction off), inv = 2 / (hi - lo)"""
    lo, hi = np.asarray(aabb[0], dtype=f32), np.asarray(aabb[1], dtype=f32)
    inv = (f32(2.0) / (hi - lo)).astype(f32)
    with np.errstate(over="ignore", invalid="ignore"):
        u = (((xn + f32(1.0)).astype(f32) / inv).astype(f32) + lo).astype(f32)
        return (((u - lo).astype(f32) * inv).astype(f32) - f32(1.0)).astype(f32)


def _dyn_reference(dy, sets, grid, xn, t):
    """float64 composition as tests/_point_prim.point_reference: features at the warped point (layer5 = 0: the float32 round
    trip of xn) | xn, PE10(xn), t, PE8(t) -> 64 -> 1 for the two heads, basis_mat on the 216 appearance features"""
    sd = {k: v.detach().cpu().double().numpy() for k, v in dy.state_dict().items()}
    xw = _round_trip(np.asarray(xn, dtype=f32), AABB)
    x0, x1, _, _ = G.encodings_reference(xn, t)
    tail = np.concatenate([x0, x1], -1)                                   # [xn 3 | sin 30 | cos 30 | t | sin 8 | cos 8]
    out = {}
    for name, (planes, lines) in zip(("density", "blending"), sets["den"]):
        feat = G.gather_reference("DYN_DENSITY", planes, lines, grid, xw)[0]
        h = np.maximum(np.concatenate([feat, tail], -1) @ sd[name + "_layer1.weight"].T + sd[name + "_layer1.bias"], 0.0)
        out[name] = (h @ sd[name + "_layer2.weight"].T + sd[name + "_layer2.bias"])[:, 0]
    out["app"] = G.gather_reference("DYN_APP", *sets["app"], grid, xw)[0] @ sd["basis_mat.weight"].T
    return out


@pytest.mark.parametrize("how,grid", [("exact", g) for g in G.EXACT_GRIDS] + [("dense", g) for g in G.DENSE_GRIDS], ids=str)
def test_dynamic_feature_entry_points(how, grid):
    import rodynrf
    case = G.exact_case if how == "exact" else G.dense_case
    cd, ca = case("DYN_DENSITY", grid), case("DYN_APP", grid)
    torch.manual_seed(7)
    dy = rodynrf.TensorVMSplit_TimeEmbedding(torch.tensor(AABB), list(grid), 12, "cuda", shadingMode="MLP_Fea_late_view", fea_pe=0, **KW)
    _load_set(dy, "density", *cd["sets"][0])
    _load_set(dy, "blending", *cd["sets"][1])
    _load_set(dy, "app", *ca["sets"][0])
    with torch.no_grad():
        dy.layer5.weight.zero_()
        dy.layer5.bias.zero_()
    dy.invalidate_packed()
    xn = cd["xn"]
    xn = xn[np.isfinite(xn).all(-1) & (np.abs(xn) <= 3.0).all(-1)]      # the encodings' own edges are the encodings tests'
    t = (np.arange(len(xn)) % 12).astype(f32) * f32(2.0 / 11.0) - f32(1.0)
    ref = _dyn_reference(dy, dict(den=cd["sets"], app=ca["sets"][0]), grid, xn, t)
    x, tt = torch.from_numpy(np.ascontiguousarray(xn)).cuda(), torch.from_numpy(t).cuda()
    with torch.no_grad():
        got = dict(density=dy.compute_densityfeature(x, tt), blending=dy.compute_blendingfeature(x, tt), app=dy.compute_appfeature(x, tt))
    for k, v in got.items():
        ex = elementwise_excess(v, torch.from_numpy(ref[k]), *FWD_ELEM)
        record_margin(f"dynamic_features_fwd {k} {how} {grid}", ex)
        assert ex <= 1.0, f"{k} {how} {grid}: element-wise |err| exceeds {FWD_ELEM[0]:.0e} |ref| + {FWD_ELEM[1]:.0e} max|ref| by a factor {ex:.2f}"


# ---- encodings ---------------------------------------------------------------------------------------------------------------
def _run_encodings(xn, t):
    L = pkg()
    xn = np.ascontiguousarray(xn, dtype=f32).reshape(-1, 3)
    t = np.ascontiguousarray(t, dtype=f32).reshape(-1)
    M = len(t)
    x, tt = torch.from_numpy(xn).cuda(), torch.from_numpy(t).cuda()
    x0 = torch.full((M * 64 + 64,), GUARD, device="cuda")
    x1 = torch.full((M * 16 + 64,), GUARD, device="cuda")
    L.check(L.lib.rdrf_selftest_encodings(L.ptr(x), L.ptr(tt), M, L.ptr(x0), L.ptr(x1), L.stream_of(x0)), "rdrf_selftest_encodings")
    x0, x1 = x0.cpu().numpy(), x1.cpu().numpy()
    assert (x0[M * 64:] == GUARD).all() and (x1[M * 16:] == GUARD).all()
    return x0[: M * 64].reshape(M, 64), x1[: M * 16].reshape(M, 16)


def _tame_points(M, rng):
    tiny = f32(2.0 ** -126)
    below = np.nextafter(f32(1.0), f32(0.0))
    xs = [0.0, 1.0, -1.0, tiny, -tiny, below, -below] + list(rng.uniform(-1.5, 1.5, 16))
    ts = [-1.0, 0.0, 1.0] + [i * 2.0 / 11.0 - 1.0 for i in range(12)]
    xn = np.stack([rng.permutation(np.resize(np.asarray(xs, dtype=f32), M)) for _ in range(3)], -1)
    return xn, rng.permutation(np.resize(np.asarray(ts, dtype=f32), M))


def _check_encodings(tag, xn, t):
    M = len(t)
    x0, x1 = _run_encodings(xn, t)
    r0, r1, w0, w1 = G.encodings_reference(xn, t)
    xn32, t32 = np.asarray(xn, dtype=f32).reshape(-1, 3), np.asarray(t, dtype=f32)
    assert np.array_equal(x0[:, :3].view(np.uint32), xn32.view(np.uint32)) and np.array_equal(x0[:, 63].view(np.uint32), t32.view(np.uint32)), \
        f"{tag}: the pass-through slots xn, t must keep their bits"
    for name, got, ref, wild in (("x0", x0[:, 3:63], r0[:, 3:63], w0), ("x1", x1, r1, w1)):
        ocml = G.wave_any(wild, M)
        bound = np.where(ocml, G.PE_OCML_BOUND, G.PE_FAST_BOUND)[:, None]
        ratio = float((np.abs(got.astype(np.float64) - ref) / bound).max())
        record_margin(f"encodings {tag} {name}", ratio)
        assert ratio <= 1.0, f"{tag} {name}: |err| is {ratio:.3f} x the bound ({int(ocml.sum())} of {M} points on the OCML path)"
    return w0, w1


@pytest.mark.parametrize("M", (1, 33, 65))
def test_encodings_fast_path(M):
    """every argument of every lane at most 1e5: sincos_pe; the switch values themselves (|xn| 512 = 1e5 and |t| 128 = 1e5 exactly,
    `<=`) and their float32 neighbours below stay on it"""
    rng = np.random.default_rng(31 + M)
    xn, t = _tame_points(M, rng)
    w0, w1 = _check_encodings(f"tame M={M}", xn, t)
    assert not w0.any() and not w1.any()
    x, tt = f32(195.3125), f32(781.25)
    xn[0] = (x, -np.nextafter(x, f32(0)), 0.5)
    t[0] = -tt
    if M > 1:
        xn[M - 1] = (-x, 0.25, np.nextafter(x, f32(0)))
        t[M - 1] = np.nextafter(tt, f32(0))
    w0, w1 = _check_encodings(f"switch values M={M}", xn, t)
    assert not w0.any() and not w1.any()


@pytest.mark.parametrize("M", (1, 33, 65))
@pytest.mark.parametrize("slot", (3, 31))
def test_encodings_wild_lane_sends_its_wave_through_ocml(M, slot):
    """one wild point (its two lanes, one per half-wave) among tame ones: the float32 neighbour above the switch value in x or in t,
    and a far argument; every lane of that wave is held to 4 ulp of 1, the other waves to the fast path's bound"""
    rng = np.random.default_rng(37 + M + slot)
    x, tt = f32(195.3125), f32(781.25)
    for which in ("x", "t", "far"):
        xn, t = _tame_points(M, rng)
        i = min(slot, M - 1) if M < 65 else 32 + slot      # M = 65: the middle wave is wild, its neighbours stay tame
        if which == "x":
            xn[i, rng.integers(0, 3)] = -np.nextafter(x, f32(1e9))
        elif which == "t":
            t[i] = np.nextafter(tt, f32(1e9))
        else:
            xn[i, 1], t[i] = f32(3.0e4), f32(-2.0e4)
        w0, w1 = _check_encodings(f"wild {which} M={M} slot={slot}", xn, t)
        assert w0.sum() == (which != "t") and w1.sum() == (which != "x")
