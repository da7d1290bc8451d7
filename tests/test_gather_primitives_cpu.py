"""The numpy reference of the forward VM gather and of the positional encodings (tests/_gather_prim.py) held to independent
statements of the same operations, without a GPU: torch.nn.functional.grid_sample in float64, the reference-generated goldens, and
the arithmetic facts the GPU file's exact and zero cases rest on (tests/test_gpu_gather_primitives.py runs the same cases)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _gather_prim as G
from _scatter_prim import AXES, HeadroomError, plane_dims, sub
from _util import CASES, RTOL, assert_close, load_case

ALL_GRIDS = G.EXACT_GRIDS + G.DENSE_GRIDS


def _lattice_points(grid, nlv, rng, n=160):
    """coordinates m / 1024 in [-1.1, 1.1]: c + 1, its half and the product with Ls - 1 <= 43 are exact in float32, so the float32
    taps of the reference and the float64 taps of grid_sample are the same numbers; a point closer than 1e-3 texel to a texel
    boundary of any level on any axis is dropped (there a tap of weight ~0 may sit on either side)"""
    pts = rng.integers(-1126, 1127, (4 * n, 3)) / 1024.0
    keep = np.ones(len(pts), dtype=bool)
    for a, g in enumerate(grid):
        for lv in range(nlv):
            if sub(g, lv) == 1:      # an axis of one texel: the position is 0 for every coordinate, one tap of weight 1
                continue
            f = (pts[:, a] + 1.0) / 2.0 * (sub(g, lv) - 1)
            keep &= np.abs(f - np.rint(f)) >= 1e-3
    pts = pts[keep][:n]
    assert len(pts) >= n // 2
    return pts.astype(np.float32)


def _grid_sample_features(kind, planes, lines, grid, xn):
    x = torch.from_numpy(np.asarray(xn, dtype=np.float64))
    out = []
    for lv in range(G.levels(kind)):
        s = 1 << lv
        for p in range(3):
            ax, ay, al = AXES[p]
            pl = torch.from_numpy(planes[p][::s, ::s].copy()).permute(2, 0, 1)[None]            # (1, C, Hs, Ws)
            ln = torch.from_numpy(lines[p][::s].copy()).permute(1, 0)[None, :, :, None]        # (1, C, Ls, 1)
            gp = torch.stack([x[:, ax], x[:, ay]], -1).view(1, -1, 1, 2)
            gl = torch.stack([torch.zeros_like(x[:, al]), x[:, al]], -1).view(1, -1, 1, 2)
            pc = F.grid_sample(pl, gp, mode="bilinear", padding_mode="zeros", align_corners=True)[0, :, :, 0]
            lc = F.grid_sample(ln, gl, mode="bilinear", padding_mode="zeros", align_corners=True)[0, :, :, 0]
            out.append((pc * lc).T)
    return torch.cat(out, -1).numpy()


@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("grid", ALL_GRIDS, ids=str)
def test_reference_equals_grid_sample_float64(kind, grid):
    rng = np.random.default_rng([17, G.KINDS.index(kind), *grid])
    (planes, lines), = G.make_sets(kind, grid, rng, "normal")
    xn = _lattice_points(grid, G.levels(kind), rng)
    feat, P, Lm = G.gather_reference(kind, planes, lines, grid, xn)
    want = _grid_sample_features(kind, planes, lines, grid, xn)
    assert feat.shape == want.shape == (len(xn), G.nfeat(kind))
    assert (np.abs(feat - want) <= 1e-12 * P * Lm).all(), float((np.abs(feat - want) / (P * Lm + 1e-300)).max())
    assert (P * Lm > 0).mean() > 0.5      # the comparison is not one of zeros


def test_level_sizes_of_the_tiny_grids():
    assert [G.level_sizes((2, 3, 5), lv) for lv in range(3)] == [(2, 3, 5), (1, 2, 3), (1, 1, 2)]
    assert [G.level_sizes((4, 2, 6), lv) for lv in range(3)] == [(4, 2, 6), (2, 1, 3), (1, 1, 2)]
    for grid in G.EXACT_GRIDS:       # Ls - 1 is a power of two or 0 at all three levels
        for lv in range(3):
            for s in G.level_sizes(grid, lv):
                assert s == 1 or (s - 1) & (s - 2) == 0, (grid, lv, s)


@pytest.mark.parametrize("name", CASES)
def test_reference_reproduces_the_goldens_static_features(name):
    g, sd_s, _, _, _ = load_case(name)
    grid = [int(v) for v in g["meta.grid"]]
    xn = g["fn.xn"]
    feat, P, Lm = G.gather_reference("STATIC_DENSITY", *G.from_state_dict(sd_s, "density"), grid, xn)
    assert_close(G.static_density(feat, P, Lm)[0], g["fn.s_density"], "s_density", rtol=RTOL)
    app = G.gather_reference("STATIC_APP", *G.from_state_dict(sd_s, "app"), grid, xn)[0]
    assert_close(app @ sd_s["basis_mat.weight"].double().numpy().T, g["fn.s_app"], "s_app", rtol=RTOL)


@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("grid", G.EXACT_GRIDS, ids=str)
def test_exact_cases_are_exact(kind, grid):
    """exact_case runs exact_check on every factor set: all eight terms of every output multiples of 2^-q, sum |terms| 2^q < 2^24"""
    c = G.exact_case(kind, grid)
    assert len(c["xn"]) == max(G.MS) and len(c["sets"]) == G.nsets_of(kind)
    flat = np.concatenate([p.ravel() for pl, _ in c["sets"] for p in pl])
    assert len(np.unique(flat)) == len(flat) and (flat == np.rint(flat)).all() and (flat != 0).all()      # distinct integers
    flat = np.concatenate([l.ravel() for _, ln in c["sets"] for l in ln])
    assert len(np.unique(flat)) == len(flat) and (flat == np.rint(flat)).all() and (flat != 0).all()
    xn = c["xn"].astype(np.float64)
    assert (np.abs(xn) == 1.0).any(), "no point on a face"
    assert (np.abs(xn) > 1.0).any() and (np.abs(xn) < 1.0).any()
    f0 = (xn + 1.0) / 2.0 * (np.asarray(grid) - 1)
    assert (G.frac_bits(f0) == 0).any() and (c["budget"] == 0 or (G.frac_bits(f0) > 0).any())
    for feat in c["ref"]:
        assert (feat != 0).mean() > 0.5


def test_headroom_error_is_raised_where_a_partial_sum_could_round():
    kind, grid = "DYN_APP", (17, 9, 5)
    c = G.exact_case(kind, grid)
    (planes, lines), = c["sets"]
    xn = np.array([[-1.0 + 2.0 * 3.25 / 16, -1.0 + 2.0 * 2.25 / 8, -1.0 + 2.0 * 1.25 / 4]], dtype=np.float32)   # quarter texels of level 0
    with pytest.raises(HeadroomError):
        G.exact_check(kind, planes, lines, grid, xn)
    big = [p * 4096.0 for p in planes]
    with pytest.raises(HeadroomError):
        G.exact_check(kind, big, lines, grid, c["xn"][:8])


@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("grid", ALL_GRIDS, ids=str)
def test_non_finite_and_far_outside_points_are_exactly_zero(kind, grid):
    """zero padding: a non-finite coordinate gives every feature of the point exactly 0.0; a coordinate beyond the padding ramp
    gives 0.0 to every feature of a level at which its axis has two texels or more (an axis of ONE texel has no outside: under
    align_corners=True every finite coordinate is that texel, in ATen as here)"""
    rng = np.random.default_rng([19, G.KINDS.index(kind), *grid])
    (planes, lines), = G.make_sets(kind, grid, rng, "normal")
    feat = G.gather_reference(kind, planes, lines, grid, np.asarray(G.NONFINITE, dtype=np.float32))[0]
    assert (feat == 0.0).all()
    far = np.asarray(G.FAR, dtype=np.float32)
    feat = G.gather_reference(kind, planes, lines, grid, far)[0]
    C = G.comps(kind)
    f0 = 0
    for lv in range(G.levels(kind)):
        sizes = G.level_sizes(grid, lv)
        out = np.array([[abs(float(c)) >= 1.0 + 2.0 / max(sizes[a] - 1, 1) and sizes[a] >= 2 for a, c in enumerate(pt)] for pt in far]).any(-1)
        for p in range(3):
            assert (feat[out, f0:f0 + C[p]] == 0.0).all(), (lv, p)
            f0 += C[p]
    inside = np.asarray([[0.25, -0.5, 0.125]], dtype=np.float32)
    assert (G.gather_reference(kind, planes, lines, grid, inside)[0] != 0.0).all()


@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("grid", G.DENSE_GRIDS, ids=str)
def test_dense_cases_hold_every_edge_coordinate(kind, grid):
    c = G.dense_case(kind, grid)
    xn = c["xn"]
    for a, g in enumerate(grid):
        col = set(xn[:, a].tolist())
        one = np.float32(1.0)
        for v in (one, -one, np.nextafter(one, np.float32(2)), np.nextafter(one, np.float32(0)), np.nextafter(-one, np.float32(-2)),
                  np.nextafter(-one, np.float32(0)), 1.5, -3.0, 1e6, -1e6, np.float32(1e30), np.float32(-1e30)):
            assert float(v) in col, (a, v)
        for lv in range(G.levels(kind)):
            Ls = sub(g, lv)
            if Ls < 2:
                continue
            for i in range(Ls):
                t = np.float32(-1.0 + 2.0 * i / (Ls - 1))
                assert {float(t), float(np.nextafter(t, np.float32(2))), float(np.nextafter(t, np.float32(-2)))} <= col, (a, lv, i)
            ramp = (np.abs(xn[:, a]) > 1) & (np.abs(xn[:, a]) < 1 + 2.0 / (Ls - 1))
            assert (xn[ramp, a] > 0).any() and (xn[ramp, a] < 0).any(), (a, lv)
    feat, P, Lm = c["ref"][0]
    assert np.isfinite(feat).all() and (P * Lm >= np.abs(feat) * (1 - 1e-12)).all()


def test_encodings_reference_layout_and_switches():
    f = np.float32
    x = f(195.3125)     # 195.3125 * 512 = 1e5 exactly: the fast path by `<=`
    tt = f(781.25)      # 781.25 * 128 = 1e5
    assert float(x) * 512 == 1e5 == float(tt) * 128
    xn = np.array([[x, 0, 0], [np.nextafter(x, f(1e9)), 0, 0], [np.nextafter(x, f(0)), 0, 0], [0, -x, 0], [0, 0, -np.nextafter(x, f(1e9))],
                   [0.5, -0.25, 1.0]], dtype=f)
    t = np.array([tt, 0, np.nextafter(tt, f(1e9)), -tt, -np.nextafter(tt, f(1e9)), 0.5], dtype=f)
    x0, x1, w0, w1 = G.encodings_reference(xn, t)
    assert w0.tolist() == [False, True, False, False, True, False]
    assert w1.tolist() == [False, False, True, False, True, False]
    assert x0.shape == (6, 64) and x1.shape == (6, 16)
    assert np.array_equal(x0[:, :3], xn.astype(np.float64)) and np.array_equal(x0[:, 63], t.astype(np.float64))
    # the oracle's order: positional_encoding(xn, 10) = [sin(q), cos(q)], q[d * 10 + k] = xn[d] 2^k
    from oracle import rodynrf_oracle as O
    pe = O.positional_encoding(torch.from_numpy(xn[5:6].astype(np.float64)), 10).numpy()
    assert np.allclose(x0[5, 3:63], pe[0], rtol=0, atol=1e-15)
    pe = O.positional_encoding(torch.from_numpy(t[5:6].astype(np.float64))[:, None], 8).numpy()
    assert np.allclose(x1[5], pe[0], rtol=0, atol=1e-15)
    assert G.wave_any(np.array([True] + [False] * 32), 33).tolist() == [True] * 33      # the tail wave's idle lanes hold point 0
    assert G.wave_any(np.array([False] * 32 + [True] + [False] * 32), 65).tolist() == [False] * 32 + [True] * 32 + [False]
