"""Reference of the forward VM gather (rdrf_selftest_gather: tap1d, axis_tap, point_taps, plane_taps, plane_taps_xz_or_yz,
taps_quads / taps_quads3, gather_level_den, gather_level_app, static_density_feature) and of the positional encodings
(rdrf_selftest_encodings: sincos_pe, fill_x0, fill_x1), in plain numpy.

The operation, per stride level lv (s = 1 << lv) and plane p with its partner line: grid_sample with align_corners=True and zero
padding on plane[::s, ::s] (bilinear) and line[::s] (linear), feature = plane_interp * line_interp.  Tap index, weights and validity
come from _scatter_prim.tap1d (float32 in tap1d's operation order, which is ATen's); everything behind the taps is float64 on those
float32 weights:  feature = (sum_ij v_ij wx_i wy_j) (sum_k a_k wl_k), with the magnitudes P = sum_ij |v_ij| wx_i wy_j and
Lm = sum_k |a_k| wl_k that the rounding bounds of tests/test_gpu_gather_primitives.py are stated in.  Logical feature order:
[level][plane][component], the order of the reference's feature vector and of the first-layer weight columns.

Exact class (exact_check): every term v_ij a_k wx_i wy_j wl_k of an output is a multiple of 2^-q, q <= Q the smallest that holds, and
sum |terms| 2^q < 2^24, so every partial sum in every order, with or without fma, is exact in fp32 (_scatter_prim.HeadroomError)."""
import numpy as np

from _scatter_prim import AXES, HeadroomError, Q, plane_dims, sub, tap1d

f32 = np.float32
U = 2.0 ** -24
KINDS = ("STATIC_DENSITY", "STATIC_APP", "DYN_DENSITY", "DYN_APP")
#        components of (XY, XZ, YZ), stride levels
SPEC = {"STATIC_DENSITY": ((16, 4, 4), 1), "STATIC_APP": ((48, 12, 12), 1), "DYN_DENSITY": ((16, 4, 4), 3), "DYN_APP": ((48, 12, 12), 3)}
PE_FAST_MAX = 1.0e5          # csrc/rdrf_common.hpp RDRF_PE_FAST_MAX: above it a wave's encodings go through OCML
PE_FAST_BOUND = 1.2e-7       # tests/test_abi_cpu.py::test_sincos_pe_formula: max abs error of sincos_pe up to the hand-over
PE_OCML_BOUND = 4 * 2.0 ** -23   # OpenCL: sin / cos within 4 ulp; |result| <= 1, so 4 ulp of 1


def comps(kind):
    return SPEC[kind][0]


def levels(kind):
    return SPEC[kind][1]


def nfeat(kind):
    return sum(comps(kind)) * levels(kind)


def level_sizes(grid, lv):
    return tuple(sub(g, lv) for g in grid)


# ---- factor sets -------------------------------------------------------------------------------------------------------------
def make_sets(kind, grid, rng, how, nsets=1):
    """nsets x (planes[p] [H][W][C], lines[p] [L][C]) (float64).  how = "normal": seeded normal data; "distinct": non-zero integers
    of both signs, the smallest that do it, no two plane entries of any set alike and no two line entries alike, dealt out in
    random order: one wrong tap, plane, quad, component or set changes the result."""
    C = comps(kind)
    dims = plane_dims(grid)
    pshape = [(H, W, C[p]) for p, (W, H, _) in enumerate(dims)] * nsets
    lshape = [(Ln, C[p]) for p, (_, _, Ln) in enumerate(dims)] * nsets

    def deal(shapes):
        n = sum(int(np.prod(s)) for s in shapes)
        if how == "normal":
            vals = rng.standard_normal(n)
        else:
            vals = np.arange(n) - n // 2
            vals = rng.permutation(np.where(vals >= 0, vals + 1, vals)).astype(np.float64)    # -n/2 .. -1, 1 .. ceil(n/2)
        out, o = [], 0
        for s in shapes:
            k = int(np.prod(s))
            out.append(vals[o:o + k].reshape(s))
            o += k
        return out
    planes, lines = deal(pshape), deal(lshape)
    return [(planes[3 * i:3 * i + 3], lines[3 * i:3 * i + 3]) for i in range(nsets)]


def from_state_dict(sd, prefix):
    """the factor set `prefix` of a golden state dict ((1, C, H, W) planes, (1, C, L, 1) lines) in this module's layout"""
    planes = [sd[f"{prefix}_plane.{p}"][0].permute(1, 2, 0).double().numpy() for p in range(3)]
    lines = [sd[f"{prefix}_line.{p}"][0, :, :, 0].permute(1, 0).double().numpy() for p in range(3)]
    return planes, lines


# ---- the gather --------------------------------------------------------------------------------------------------------------
def gather_terms(kind, planes, lines, grid, xn):
    """per feature, in logical order: the four plane taps and two line taps behind it.
    -> v [M][F][4], wp [M][F][4] (wx_i wy_j, exact products of the float32 weights), a [M][F][2], wl [M][F][2], all float64"""
    xn = np.asarray(xn, dtype=f32).reshape(-1, 3)
    M, F = xn.shape[0], nfeat(kind)
    v, wp = np.zeros((M, F, 4)), np.zeros((M, F, 4))
    a, wl = np.zeros((M, F, 2)), np.zeros((M, F, 2))
    f0 = 0
    for lv in range(levels(kind)):
        for p, (W, H, Ln) in enumerate(plane_dims(grid)):
            ax, ay, al = AXES[p]
            Ws, Hs, Ls = sub(W, lv), sub(H, lv), sub(Ln, lv)
            ix, wx0, wx1, _, _ = tap1d(xn[:, ax], Ws)       # weights of out-of-range taps are 0 (zero padding)
            iy, wy0, wy1, _, _ = tap1d(xn[:, ay], Hs)
            il, wl0, wl1, _, _ = tap1d(xn[:, al], Ls)
            plane = np.asarray(planes[p], dtype=np.float64)[:: 1 << lv, :: 1 << lv]
            line = np.asarray(lines[p], dtype=np.float64)[:: 1 << lv]
            assert plane.shape[:2] == (Hs, Ws) and line.shape[0] == Ls
            Cn = plane.shape[2]
            sl = slice(f0, f0 + Cn)
            cx = lambda i: np.clip(i, 0, Ws - 1)
            cy = lambda i: np.clip(i, 0, Hs - 1)
            cl = lambda i: np.clip(i, 0, Ls - 1)
            wx0, wx1, wy0, wy1 = (w.astype(np.float64) for w in (wx0, wx1, wy0, wy1))
            for k, (yy, xx, w) in enumerate(((iy, ix, wx0 * wy0), (iy, ix + 1, wx1 * wy0), (iy + 1, ix, wx0 * wy1), (iy + 1, ix + 1, wx1 * wy1))):
                v[:, sl, k] = plane[cy(yy), cx(xx)]
                wp[:, sl, k] = w[:, None]
            for k, (ll, w) in enumerate(((il, wl0), (il + 1, wl1))):
                a[:, sl, k] = line[cl(ll)]
                wl[:, sl, k] = w.astype(np.float64)[:, None]
            f0 += Cn
    assert f0 == F
    return v, wp, a, wl


def gather_reference(kind, planes, lines, grid, xn):
    """-> (features [M][F] float64, P [M][F], Lm [M][F]); STATIC_DENSITY callers sum the features (static_density)"""
    v, wp, a, wl = gather_terms(kind, planes, lines, grid, xn)
    return (v * wp).sum(-1) * (a * wl).sum(-1), (np.abs(v) * wp).sum(-1), (np.abs(a) * wl).sum(-1)


def static_density(feat, P, Lm):
    """the static field's density feature: the sum of its 24 products, and the magnitude sum_f P_f Lm_f of its bound"""
    return feat.sum(-1), (P * Lm).sum(-1)


def exact_check(kind, planes, lines, grid, xn):
    """the exact class: features as int64 fixed point.  Raises HeadroomError unless every one of the eight terms of every output
    (and, for STATIC_DENSITY, of the 24-product sum) is a multiple of 2^-q and sum |terms| 2^q < 2^24.  -> features [M][F] float64"""
    v, wp, a, wl = gather_terms(kind, planes, lines, grid, xn)
    terms = (v * wp)[..., :, None] * (a * wl)[..., None, :]            # [M][F][4][2]
    terms = terms.reshape(terms.shape[0], terms.shape[1], 8)
    if kind == "STATIC_DENSITY":
        terms = terms.reshape(terms.shape[0], 1, -1)
    out = np.zeros(terms.shape[:2])
    for m in range(terms.shape[0]):
        for q in range(Q + 1):
            t = terms[m] * 2.0 ** q
            if (t == np.rint(t)).all():
                break
        else:
            raise HeadroomError(f"{kind} point {m}: a term is not a multiple of 2^-{Q}")
        ti = np.rint(t).astype(np.int64)
        mag = np.abs(ti).sum(-1)
        if mag.max() >= 2 ** 24:
            raise HeadroomError(f"{kind} point {m}: sum |terms| 2^{q} = {mag.max()} >= 2^24: a partial sum may round in fp32")
        out[m] = ti.sum(-1) / 2.0 ** q
    feat = gather_reference(kind, planes, lines, grid, xn)[0]
    ref = feat.sum(-1, keepdims=True) if kind == "STATIC_DENSITY" else feat
    assert np.array_equal(out, ref), "the float64 evaluation of an exact case must be exact as well"
    return feat


# ---- coordinates -------------------------------------------------------------------------------------------------------------
def frac_bits(x):
    """fractional bits of the dyadic numbers x (at most 8)"""
    x = np.asarray(x, dtype=np.float64)
    b = np.zeros(x.shape, dtype=np.int64)
    for k in range(1, 9):
        b = np.where((x * 2.0 ** (k - 1)) != np.rint(x * 2.0 ** (k - 1)), k, b)
    return b


def exact_budget(kind, sets):
    """largest q with max |v| max |a| 2^q n < 2^24 (n products per output: 1, or 24 for the static density sum): the interpolation
    weights of an output sum to at most 1, so sum |terms| <= max |v| max |a| whatever the position"""
    vmax = max(float(np.abs(p).max()) for ps, _ in sets for p in ps)
    amax = max(float(np.abs(l).max()) for _, ls in sets for l in ls)
    n = 24 if kind == "STATIC_DENSITY" else 1
    q = 0
    while vmax * amax * n * 2.0 ** (q + 1) < 2 ** 24 and q < Q:
        q += 1
    assert vmax * amax * n * 2.0 ** q < 2 ** 24, "no headroom at all: the grid is too large for distinct integers"
    return q


def exact_coords(kind, grid, n, budget, rng):
    """n points for a 2^k + 1 grid: per axis a level-0 texel coordinate f = m / 4 (texel-aligned, half- and quarter-texel positions of
    level 0, which contain those of levels 1 and 2), up to 1.5 texels of the deepest level outside the box, the faces among them;
    a draw is kept when the fractional bits of its three tap positions add up to at most `budget` at every level
    (exact_budget), drawn so that every class that fits is present: aligned at every level, half / quarter texel of level 2, of
    level 1, of level 0, on one, two or three axes."""
    nlv = levels(kind)
    ks = []
    for g in grid:
        k = int(np.log2(g - 1))
        assert (1 << k) + 1 == g, "the exact cases need 2^k + 1 grids"
        ks.append(k)
    out = np.zeros((n, 3))
    got = 0
    steps = (16, 8, 4, 2, 1)      # f is a multiple of step / 4: aligned at level 2, 1, 0, half, quarter texel of level 0
    guard = 0
    while got < n:
        guard += 1
        assert guard < 100000, "exact_coords: the budget admits too few positions"
        f = np.zeros(3)
        for a in range(3):
            Lm1 = 1 << ks[a]
            r = rng.random()
            if r < 0.15:
                f[a] = rng.choice([0.0, float(Lm1)])                      # a face
            else:
                st = steps[rng.choice(len(steps), p=(0.1, 0.15, 0.25, 0.25, 0.25))]
                out4 = 0 if r < 0.8 else 6 << (nlv - 1)     # one point in five may lie outside, up to 1.5 texels of the deepest level
                f[a] = rng.integers(-(out4 // st), (4 * Lm1 + out4) // st + 1) * st / 4.0
        bits = max(sum(int(frac_bits(f[a] * (sub(grid[a], lv) - 1) / (1 << ks[a]))) for a in range(3)) for lv in range(nlv))
        if bits > budget:
            continue
        out[got] = [-1.0 + 2.0 * f[a] / (1 << ks[a]) for a in range(3)]
        got += 1
    assert np.array_equal(out.astype(f32).astype(np.float64), out)
    return out.astype(f32)


def dense_axis_pool(L, nlv, rng, n_uniform=8):
    """the edge coordinates of one axis of L texels (float32): uniform in [-1.1, 1.1]; +-1, their float32 neighbours on both sides;
    every texel centre of every level as the nearest float32 and its two float32 neighbours; the padding ramp
    1 < |c| < 1 + 2 / (Ls - 1) of every level; |c| in {1.5, 3, 1e6, 1e30}"""
    vals = list(rng.uniform(-1.1, 1.1, n_uniform).astype(f32))
    for s in (-1.0, 1.0):
        one = f32(s)
        vals += [one, np.nextafter(one, f32(s * np.inf)), np.nextafter(one, f32(0))]
        vals += [f32(s * b) for b in (1.5, 3.0, 1e6, 1e30)]
    for lv in range(nlv):
        Ls = sub(L, lv)
        if Ls < 2:
            continue
        for i in range(Ls):
            c = f32(-1.0 + 2.0 * i / (Ls - 1))
            vals += [c, np.nextafter(c, f32(np.inf)), np.nextafter(c, f32(-np.inf))]
        w = 2.0 / (Ls - 1)
        for s in (-1.0, 1.0):
            vals += [f32(s * (1.0 + w * r)) for r in rng.uniform(0.02, 0.98, 2)]
    return np.asarray(vals, dtype=f32)


def dense_coords(grid, nlv, rng, n_combo=97):
    """every pool value of every axis once with the other two coordinates inside the box (else the zero of a far-outside axis would
    hide it), then n_combo points drawing all three coordinates from the pools"""
    pools = [dense_axis_pool(g, nlv, rng) for g in grid]
    pts = []
    for a in range(3):
        p = np.empty((len(pools[a]), 3), dtype=f32)
        p[:] = rng.uniform(-1.0, 1.0, p.shape).astype(f32)
        p[:, a] = pools[a]
        pts.append(p)
    combo = np.stack([pools[a][rng.integers(0, len(pools[a]), n_combo)] for a in range(3)], -1)
    return rng.permutation(np.concatenate(pts + [combo]), axis=0)


NONFINITE = [(np.nan, 0.25, -0.5), (0.25, np.inf, -0.5), (0.25, -0.5, -np.inf), (np.nan, np.inf, 0.1), (0.1, -np.inf, np.nan),
             (np.inf, 0.3, np.nan), (np.nan, np.nan, np.nan), (np.inf, np.inf, np.inf), (-np.inf, np.nan, np.inf),
             (-np.inf, -np.inf, -np.inf)]
FAR = [(1e30, 0.0, 0.0), (0.0, -1e6, 0.5), (0.5, 0.5, 3.0), (-1.5, 1.5, 1e30), (1e30, 1e30, 1e30), (-1e6, 3.0, -1e30)]


# ---- the cases of tests/test_gpu_gather_primitives.py (tests/test_gather_primitives_cpu.py checks the reference on the same) ---------
EXACT_GRIDS = ((17, 9, 5), (5, 17, 3), (3, 3, 3))
DENSE_GRIDS = ((6, 7, 11), (40, 44, 26), (2, 3, 5), (4, 2, 6))
MS = (1, 31, 32, 33, 65, 97)
_CASES = {}


def nsets_of(kind):
    return 2 if kind == "DYN_DENSITY" else 1       # the density and the blending set go through the same device function


def exact_case(kind, grid):
    """distinct integers, 97 dyadic points inside the kind's headroom; computed once, shared, never modified"""
    key = ("exact", kind, tuple(grid))
    if key not in _CASES:
        rng = np.random.default_rng([3, KINDS.index(kind), *grid])
        sets = make_sets(kind, grid, rng, "distinct", nsets_of(kind))
        budget = exact_budget(kind, sets)
        xn = exact_coords(kind, grid, max(MS), budget, rng)
        ref = [exact_check(kind, pl, ln, grid, xn) for pl, ln in sets]
        _CASES[key] = dict(kind=kind, grid=tuple(grid), sets=sets, xn=xn, ref=ref, budget=budget)
    return _CASES[key]


def dense_case(kind, grid):
    """seeded normal data, the edge coordinates of dense_coords with the non-finite and far-outside points mixed in"""
    key = ("dense", kind, tuple(grid))
    if key not in _CASES:
        rng = np.random.default_rng([5, KINDS.index(kind), *grid])
        sets = make_sets(kind, grid, rng, "normal", nsets_of(kind))
        xn = dense_coords(grid, levels(kind), rng)
        ref = [gather_reference(kind, pl, ln, grid, xn) for pl, ln in sets]
        _CASES[key] = dict(kind=kind, grid=tuple(grid), sets=sets, xn=xn, ref=ref)
    return _CASES[key]


def batches(n, size=97):
    return [slice(i, min(i + size, n)) for i in range(0, n, size)]


# ---- encodings ---------------------------------------------------------------------------------------------------------------
def encodings_reference(xn, t):
    """-> x0 [M][64] = [xn 3 | sin(2^k xn_d) d-major, k = 0..9 | cos likewise | t], x1 [M][16] = [sin(2^k t) k = 0..7 | cos], float64
    sin / cos of the exact float32 arguments ldexp(x, k); and wild [M]: the point sends its wave through OCML (fill_x0, fill_x1)"""
    xn = np.asarray(xn, dtype=f32).reshape(-1, 3)
    t = np.asarray(t, dtype=f32).reshape(-1)
    with np.errstate(over="ignore"):
        qx = np.stack([np.ldexp(xn[:, d], k) for d in range(3) for k in range(10)], -1).astype(f32).astype(np.float64)
        qt = np.stack([np.ldexp(t, k) for k in range(8)], -1).astype(f32).astype(np.float64)
        wild0 = ~((np.abs(xn).max(-1) * f32(512.0)).astype(f32) <= f32(PE_FAST_MAX))
        wild1 = ~((np.abs(t) * f32(128.0)).astype(f32) <= f32(PE_FAST_MAX))
    x0 = np.concatenate([xn.astype(np.float64), np.sin(qx), np.cos(qx), t.astype(np.float64)[:, None]], -1)
    x1 = np.concatenate([np.sin(qt), np.cos(qt)], -1)
    return x0, x1, wild0, wild1


def wave_any(flag, M):
    """a point's wave (32 points; the lanes past M hold point 0) has a flagged lane"""
    flag = np.asarray(flag, dtype=bool)
    out = np.zeros(M, dtype=bool)
    for w0 in range(0, M, 32):
        n = min(32, M - w0)
        out[w0:w0 + n] = flag[w0:w0 + n].any() or (n < 32 and flag[0])
    return out
