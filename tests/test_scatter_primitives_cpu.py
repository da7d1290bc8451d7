"""CPU side of the stand-alone scatter / sort harness (rdrf_selftest_scatter, rdrf_selftest_sort, tests/_scatter_prim.py): the
symbols, the layout descriptions of the four kinds, and the numpy reference against float64 autograd through F.grid_sample on
strided sub-arrays (an independent formulation of the same operation)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _scatter_prim as P

from _util import pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rdrf_selftest_sort_temp_bytes", "rdrf_selftest_sort", "rdrf_selftest_scatter_workspace_bytes", "rdrf_selftest_scatter",
       "rdrf_selftest_scatter_describe", "rdrf_selftest_scatter_last")


@pytest.mark.parametrize("name", ["librodynrf.so", "librodynrf_det.so"])
def test_both_libraries_export_the_scatter_selftests(name):
    lib = C.CDLL(os.path.join(ROOT, "robust-dynrf_amd", name))
    assert all(hasattr(lib, s) for s in NEW)


def test_the_binding_lists_the_scatter_selftests():
    assert all(s in pkg().SYMBOLS for s in NEW)


def test_describe_and_host_calls_work_without_a_device():
    L = pkg()
    for kind in P.KINDS:
        d = P.describe(L, kind, [9, 17, 33])
        assert d["wk"] == [12, 12, 20] and (1 << d["kb"]) - 1 >= 20 * 36 > (1 << (d["kb"] - 1)) - 1
        assert P.describe(L, kind)["kb"] == 0
    buf = (C.c_int * 4)()
    assert L.lib.rdrf_selftest_scatter_describe(99, None, buf, 4) == -1
    assert L.lib.rdrf_selftest_scatter_describe(1, None, buf, 4) == -3
    assert L.lib.rdrf_selftest_scatter_last(buf, 4) == 4 and buf[3] == 0      # nothing launched yet
    assert L.lib.rdrf_selftest_sort_temp_bytes(4097, 18) > 2 * 4097 * 4
    assert L.lib.rdrf_selftest_scatter_workspace_bytes(4, 33) > 9 * 4 * 33 * 4


@pytest.mark.parametrize("kind", P.KINDS)
def test_every_layout_is_a_bijection_of_features_onto_rows_and_record_slots(kind):
    d = P.describe(pkg(), kind)
    fm = P.feature_map(d)
    assert len(fm) == d["nfeat"] == {"STATIC_DENSITY": 24, "DYN_DENSITY": 72, "STATIC_APP": 72, "DYN_APP": 216}[kind]
    rows = [r for r, *_ in fm]
    if d["bcast"]:
        assert set(rows) == {0}
    else:
        assert sorted(rows) == list(range(d["nfeat"]))
        for set_ in range(d["nsets"]):
            assert 0 <= d["row0"][set_] and d["row0"][set_] + d["nfeat"] <= d["stride"]
        if d["nsets"] == 2:
            assert abs(d["row0"][0] - d["row0"][1]) >= d["nfeat"]
    for lv in range(d["nlv"]):            # (level, plane) -> every component once
        for p in range(3):
            assert sorted(c for _, l, pp, c, _ in fm if l == lv and pp == p) == list(range(d["C"][p]))
    slots = [s for *_, s in fm]
    if d["rec_floats"]:
        assert sorted(slots) == list(range(d["nfeat"])) and d["set_floats"] == d["nfeat"]
        assert d["rec_floats"] == d["nsets"] * d["set_floats"]
        assert all(s % 4 == 0 for *_, s in fm[::4])                     # a quad is one aligned 16-byte load
    else:
        assert set(slots) == {-1}
    for r in d["live_rows"]:
        assert r == -1 or (0 <= r < d["stride"] and not any(d["row0"][s] <= r < d["row0"][s] + d["nfeat"] for s in range(d["nsets"])))


def _autograd(case, mode):
    """float64 autograd through F.grid_sample on plane[::s, ::s] and line[::s]"""
    d = case["desc"]
    xs = torch.from_numpy(P.normalise(case).astype(np.float64)).requires_grad_(True)
    idx, erow = P.entries(case)
    fm = P.feature_map(d)
    planes = [[torch.from_numpy(a.copy()).requires_grad_(True) for a in s] for s in case["planes"]]
    lines = [[torch.from_numpy(a.copy()).requires_grad_(True) for a in s] for s in case["lines"]]
    loss = 0.0
    x = xs[torch.from_numpy(idx)]
    for set_ in range(d["nsets"]):
        if not (case["set_mask"] >> set_) & 1:
            continue
        dq = torch.from_numpy(case["dq"][set_][erow])
        for lv in range(d["nlv"]):
            for p in range(3):
                ax, ay, al = P.AXES[p]
                st = 1 << lv
                pl = planes[set_][p][::st, ::st].permute(2, 0, 1)[None]                 # [1][C][Hs][Ws]
                ln = lines[set_][p][::st].permute(1, 0)[None, :, :, None]               # [1][C][Ls][1]
                g2 = torch.stack([x[:, ax], x[:, ay]], -1)[None, :, None, :]
                g1 = torch.stack([torch.zeros_like(x[:, al]), x[:, al]], -1)[None, :, None, :]
                pv = F.grid_sample(pl, g2, mode="bilinear", padding_mode="zeros", align_corners=True)[0, :, :, 0].T
                lv_ = F.grid_sample(ln, g1, mode="bilinear", padding_mode="zeros", align_corners=True)[0, :, :, 0].T
                feats = [f for f, (_, l, pp, _, _) in enumerate(fm) if l == lv and pp == p]
                w = dq[:, [0] * len(feats)] if d["bcast"] else dq[:, feats]
                loss = loss + (pv * lv_ * w).sum()
    loss.backward()
    out = {}
    for set_ in range(d["nsets"]):
        for p in range(3):
            g = planes[set_][p].grad
            out[("plane", set_, p)] = np.zeros(planes[set_][p].shape) if g is None else g.numpy()
            g = lines[set_][p].grad
            out[("line", set_, p)] = np.zeros(lines[set_][p].shape) if g is None else g.numpy()
    dw = xs.grad.numpy()
    dmode = d["dxw_ray"] if mode == "ray" else d["dxw_sorted"]
    out["dxw"] = dw if dmode else np.zeros_like(dw)
    out["g_xyz"] = dw * np.asarray(case["box_inv"]) if d["g_xyz"] else np.zeros_like(dw)
    return out


@pytest.mark.parametrize("kind", P.KINDS)
def test_reference_agrees_with_float64_autograd_through_grid_sample(kind):
    """non-dyadic grid, random coordinates with out-of-range ones, dead samples, an unsorted list"""
    d = P.describe(pkg(), kind, [17, 19, 11])
    rng = np.random.default_rng(5)
    N, S = 3, 37
    coords = rng.uniform(-1.3, 1.3, (N * S, 3))
    coords[5] = [1.0, -1.0, 1.0]
    coords[6] = [3.0, 0.2, 0.1]
    coords[7] = [0.2, 0.3, -1e30]
    valid = rng.random(N * S) < 0.8
    lst = rng.permutation(N * S)[:70] if d["list"] else None
    case = P.make_case(d, [17, 19, 11], N, S, coords, rng, valid=valid, list_=lst, dense=True, box_lo=(-1.5, -1.7, -1.0),
                       box_inv=(2 / 3.0, 2 / 3.4, 1.0))
    for mode in ("ray", "sorted") if d["rec_floats"] else ("ray",):
        got, mag = P.reference(case, mode, "f64")
        want = _autograd(case, mode)
        # the reference forms tap positions in float32 as the kernels do (autograd: float64): f = (c + 1) / 2 (L - 1) <= 18 carries
        # three roundings of 2^-24 relative, so a weight is off by up to 3 * 18 * 2^-24 = 3.2e-6, and a term (a product of up to three
        # weights with |values| whose sum is mag) by up to 1e-5 of the largest sum of |terms|
        for k in want:
            err = np.abs(got[k] - want[k]).max()
            assert err <= 1e-5 * max(1.0, mag[k].max()), (kind, mode, k, err)
        assert any(np.abs(want[k]).max() > 0.1 for k in want if k[0] == "plane")


def _exact_case(kind, seed=1, **kw):
    grid = [9, 17, 9]
    d = P.describe(pkg(), kind, grid)
    rng = np.random.default_rng(seed)
    N, S = 2, 33
    return P.make_case(d, grid, N, S, P.dyadic_coords(rng, grid, N * S), rng, **kw)


@pytest.mark.parametrize("kind", P.KINDS)
def test_fixed_point_path_equals_float64_on_exact_inputs(kind):
    case = _exact_case(kind, mag=1)
    pre = {k: np.random.default_rng(2).integers(-3, 4, s).astype(np.float64) for k, s in P.shapes(case).items()}
    ex, mag = P.reference(case, "ray", "exact", pre)
    fl, _ = P.reference(case, "ray", "f64", pre)
    sq, _ = P.reference(case, "ray", "seq32", pre)
    for k in ex:
        assert np.array_equal(ex[k], fl[k]) and np.array_equal(ex[k], sq[k]), k
        assert (mag[k] >= np.abs(ex[k])).all() and (ex[k] * 2 ** P.Q == np.rint(ex[k] * 2 ** P.Q)).all()
    assert any(not np.array_equal(ex[k], pre[k]) for k in ex)
    untouched = "dxw" if not case["desc"]["dxw_ray"] else "g_xyz"
    assert np.array_equal(ex[untouched], pre[untouched])


def test_headroom_assertion_fires_when_provoked():
    with pytest.raises(P.HeadroomError, match="2\\^24"):
        P.reference(_exact_case("DYN_DENSITY", mag=200), "ray", "exact")
    case = _exact_case("DYN_DENSITY", mag=1)
    case["coords"] = case["coords"] + np.float32(1 / 3.0)          # weights that are no dyadic fractions
    with pytest.raises(P.HeadroomError, match="multiple"):
        P.reference(case, "ray", "exact")


def test_overwritten_and_accumulated_coordinate_gradients_differ_only_in_the_prefill():
    case = _exact_case("DYN_APP", mag=1, list_=np.random.default_rng(0).permutation(66)[:40])
    pre = {k: np.full(s, 5.0) for k, s in P.shapes(case).items()}
    ray, _ = P.reference(case, "ray", "exact", pre)
    srt, _ = P.reference(case, "sorted", "exact", pre)
    listed = np.zeros(66, dtype=bool)
    listed[case["list"]] = True
    assert np.array_equal(srt["dxw"][listed] - 5.0, ray["dxw"][listed]) and np.array_equal(srt["dxw"][~listed], ray["dxw"][~listed])
    assert np.array_equal(ray["dxw"][~listed], pre["dxw"][~listed])


def test_keys_sort_and_counts_of_the_reference():
    grid = [9, 17, 9]
    d = P.describe(pkg(), "DYN_DENSITY", grid)
    coords = np.array([[-1, -1, -1], [1, 1, 1], [0, 0, 0], [1.0001, 0, 0], [1.6, 0, 0], [1e30, 0, 0], [0, 0, 0], [0, 0, 0]], dtype=np.float32)
    valid = np.array([1, 1, 1, 1, 1, 1, 0, 1])
    case = P.make_case(d, grid, 1, 8, coords, np.random.default_rng(0), valid=valid, sm_dead=[7])
    keys, ks, order, counts = P.reference_keys(case)
    kb, drop = d["kb"], (1 << d["kb"]) - 1
    cell = keys.reshape(3, 8) & drop
    assert cell[0, 0] == 2 * 12 + 2 and cell[0, 1] == (16 + 2) * 12 + (8 + 2) and cell[0, 2] == (8 + 2) * 12 + (4 + 2)
    assert cell[0, 3] == 10 * 12 + 10                      # just outside: the level-0 tap 8 is still in range (weight ~0 on 9)
    assert cell[0, 4] == 10 * 12 + 9 + 2                   # x = 1.6: only level 2 still has a tap; the level-0 index 10 clamps to W
    assert cell[0, 5] == drop                              # x out of range at every level
    assert cell[2, 4] != drop                              # plane YZ does not look at x
    assert (cell[:, 6] == drop).all() and (cell[:, 7] == drop).all()
    assert counts == [5, 5, 6] and (np.diff(ks.astype(np.int64)) >= 0).all()
    assert (keys >> kb).reshape(3, 8).tolist() == [[p] * 8 for p in range(3)]
    k2, o2 = P.reference_sort(np.array([3, 1, 3, 1, 2], dtype=np.uint32), 2)
    assert k2.tolist() == [1, 1, 2, 3, 3] and o2.tolist() == [1, 3, 4, 0, 2]
    k1, o1 = P.reference_sort(np.array([3, 1, 2, 0], dtype=np.uint32), 1)      # only the low bit is sorted on
    assert o1.tolist() == [2, 3, 0, 1]


def test_layouts_round_trip_through_rows_and_records():
    case = _exact_case("DYN_DENSITY", sm_dead=[3, 40])
    d = case["desc"]
    rows, recs = P.layout_rows(case), P.layout_recs(case)
    assert rows.shape == (2 * 2, d["stride"], 32) and recs.shape == (66, d["rec_floats"])
    fm = P.feature_map(d)
    s, f = 40 - 33, 17
    assert rows[2, d["row0"][1] + fm[f][0], s] == case["dq"][1][40, f] == 0.0
    assert rows[3, d["row0"][0] + fm[f][0], 0] == case["dq"][0][33 + 32, f] == recs[65, fm[f][4]]
    assert rows[0, d["live_rows"][0], 3] == 0.0 and rows[0, d["live_rows"][0], 4] == 1.0
    flat = dict(case, flat=1)
    assert P.layout_rows(flat).shape[0] == 3 and P.layout_rows(flat)[1, d["row0"][0] + fm[f][0], 1] == case["dq"][0][33, f]


DENSE_GRIDS = ([17, 19, 11], [23, 13, 29])


@pytest.mark.parametrize("grid", DENSE_GRIDS, ids=["17x19x11", "23x13x29"])
@pytest.mark.parametrize("kind", P.KINDS)
def test_fp32_sums_in_permuted_orders_against_the_sequential_one(kind, grid, capsys):
    """The dense GPU class bounds e = max |g - g64| / sum |terms| per output tensor by 2 e_seq32.  Here the same fp32 terms are
    added in three random orders, at the shapes the GPU test uses, and the ratio e_perm / e_seq32 is REPORTED per tensor.
    Finding: a permuted fp32 sum does not always stay within 2: DYN_DENSITY on 17x19x11 reaches 2.24 on the z line of the density
    set (every other tensor of every kind and grid stays below 1.9).  So the bound of 2 is not one that every legitimate fp32
    summation order meets; the kernels meet it (measured worst ratio 1.55) because run sums form in a tree and the line sums in
    fp64.  What is asserted here is what the number format guarantees for ANY order: n fp32 additions and at most 6 roundings
    inside a term give e <= (n + 6) 2^-24, n = the largest number of terms an element receives."""
    d = P.describe(pkg(), kind, grid)
    case = P.dense_case(d, grid)
    g64, mag = P.reference(case, "ray", "f64")
    tm32 = P.terms(case, np.float32)
    nmax = max(int(np.bincount(f).max()) for f, _, _ in tm32.values())
    e_seq = P.error_metric(P.reference(case, "ray", "seq32", tm=tm32)[0], g64, mag)
    worst = {}
    for seed in (1, 2, 3):
        e = P.error_metric(P.reference(case, "ray", "seq32", perm_seed=seed, tm=tm32)[0], g64, mag)
        for k in e:
            assert 0.0 < e[k] <= (nmax + 6) * 2.0 ** -24 and 0.0 < e_seq[k] <= (nmax + 6) * 2.0 ** -24, (k, e[k], e_seq[k], nmax)
            worst[k] = max(worst.get(k, 0.0), e[k] / e_seq[k])
    with capsys.disabled():
        over = {str(k): round(v, 2) for k, v in worst.items() if v > 2.0}
        print(f"\n{kind} {'x'.join(map(str, grid))}: worst e_perm / e_seq32 = {max(worst.values()):.2f}" + (f", above 2: {over}" if over else ""))
