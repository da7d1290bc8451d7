"""Reference of the gradient scatter (VM gather backward) and of the sort in front of its sorted forms, in plain numpy, built
from rdrf_selftest_scatter_describe alone (no sv:: constant is known here).

The operation, per factor set, stride level lv (s = 1 << lv) and plane p with its partner line: grid_sampler_2d_backward with
align_corners=True and zero padding on plane[::s, ::s] (bilinear) and line[::s] (linear):
    feature = plane_interp * line_interp,  d plane[tap] += dq * line_interp * w_x w_y,  d line[tap] += dq * plane_interp * w_l,
    d coordinate = dq * (line_interp * d plane_interp / dc, plane_interp * d line_interp / dc), summed over the quads.
Tap index and weights are formed in float32 in the operation order of tap1d (which is ATen's); everything behind them runs in
the dtype asked for: float64 (dense cases), float32 in sample order (the e_seq32 baseline) or int64 fixed point with Q fractional
bits (exact cases: every term must be a multiple of 2^-q, q <= Q chosen per output as the smallest that holds, and
sum |terms| 2^q < 2^24 per output element, so that every partial sum of every summation order is exact in fp32: HeadroomError)."""
import ctypes as C

import numpy as np

Q = 12                      # fractional bits of the fixed-point path
KINDS = ("STATIC_DENSITY", "DYN_DENSITY", "STATIC_APP", "DYN_APP")
# plane p samples (cx, cy) and its line cl from these coordinate axes: XY | Z, XZ | Y, YZ | X
AXES = ((0, 1, 2), (0, 2, 1), (1, 2, 0))
f32 = np.float32


def plane_dims(grid):
    """(W, H, L) of the three plane / line pairs of a factor set on grid (gx, gy, gz)"""
    return [(grid[a], grid[b], grid[c]) for a, b, c in AXES]


def describe(L, kind, grid=None):
    buf = (C.c_int * 512)()
    g = None
    if grid is not None:
        wh = [v for W, H, _ in plane_dims(grid) for v in (W, H)]
        g = (C.c_int * 6)(*wh)
    n = L.lib.rdrf_selftest_scatter_describe(L.SCATTER_KINDS[kind], g, buf, 512)
    if n < 0:
        raise RuntimeError(f"rdrf_selftest_scatter_describe {kind}: rc {n}: {L.lib.rdrf_last_error().decode()}")
    d = list(buf[:n])
    assert d[0] == n
    names = ("c0q", "c1q", "nlv", "nsets", "stride", "row0_0", "row0_1", "bcast", "rec_floats", "set_floats", "live_row0",
             "live_row1", "list", "xw", "dxw_ray", "dxw_sorted", "g_xyz", "flat", "kb", "wk0", "wk1", "wk2", "nq")
    out = dict(zip(names, d[1:24]))
    out["kind"] = kind
    out["row0"] = [out.pop("row0_0"), out.pop("row0_1")]
    out["live_rows"] = [out.pop("live_row0"), out.pop("live_row1")]
    out["wk"] = [out.pop("wk0"), out.pop("wk1"), out.pop("wk2")]
    out["quads"] = [tuple(d[24 + 5 * i: 29 + 5 * i]) for i in range(out["nq"])]   # (row, level, plane, comp0, rec offset)
    out["C"] = [16 * out["c0q"] // 4, 4 * out["c1q"], 4 * out["c1q"]]
    out["nfeat"] = 4 * out["nq"]
    return out


def feature_map(desc):
    """per feature f = 4 quad + c: (row, level, plane, component, record slot)"""
    return [(row + (0 if desc["bcast"] else c), lv, p, c0 + c, (rec + c) if rec >= 0 else -1)
            for row, lv, p, c0, rec in desc["quads"] for c in range(4)]


# ---- taps --------------------------------------------------------------------------------------------------------------------
def tap1d(c, Ls):
    """float32, the operation order of tap1d (rdrf_common.hpp) = ATen's grid_sampler_compute_source_index + floor"""
    c = np.asarray(c, dtype=f32)
    with np.errstate(over="ignore", invalid="ignore"):
        f = ((c + f32(1)) / f32(2)) * f32(Ls - 1)
        fl = np.floor(f)
        w1 = f - fl
        w0 = (fl + f32(1)) - f
        i0 = np.where(np.isnan(fl), f32(-2), np.clip(fl, f32(-2), f32(Ls + 1))).astype(np.int64)
        ok0 = (fl >= 0) & (fl <= f32(Ls - 1))
        ok1 = (fl >= -1) & (fl <= f32(Ls - 2))
    w0 = np.where(ok0, w0, f32(0))   # a tap out of range carries no weight (zero padding)
    w1 = np.where(ok1, w1, f32(0))
    return i0, w0, w1, ok0, ok1


def sub(n, lv):
    return (n + (1 << lv) - 1) >> lv


def normalise(case):
    """the coordinates the taps see, float32 (static kinds: (xyz - lo) * inv - 1, three roundings)"""
    x = np.asarray(case["coords"], dtype=f32)
    if case["desc"]["xw"]:
        return x
    lo, inv = np.asarray(case["box_lo"], dtype=f32), np.asarray(case["box_inv"], dtype=f32)
    with np.errstate(over="ignore", invalid="ignore"):
        return ((x - lo) * inv) - f32(1)


def entries(case):
    """(sample id, row of the d(feature) arrays) of every entry that scatters"""
    desc = case["desc"]
    if desc["list"]:
        idx = np.asarray(case["list"][: case["count"]], dtype=np.int64)
        return idx, np.arange(len(idx))
    idx = np.nonzero(np.asarray(case["valid"]).reshape(-1) != 0)[0]
    return idx, idx


# ---- the terms ---------------------------------------------------------------------------------------------------------------
def terms(case, dtype=np.float64):
    """every addition of the operation as (target, flat index, value, sample) arrays, grouped by target:
    ("plane", set, p), ("line", set, p) -> the logical [H][W][C] / [L][C] gradient arrays, "dw" -> [N S][3] coordinate gradients"""
    desc = case["desc"]
    xs = normalise(case)
    idx, erow = entries(case)
    out = {}

    def emit(key, flat, val, samp):
        keep = val != 0
        out.setdefault(key, []).append((flat[keep], val[keep], samp[keep]))

    fmap = feature_map(desc)
    for set_ in range(desc["nsets"]):
        if not (case["set_mask"] >> set_) & 1:
            continue
        dq_all = np.asarray(case["dq"][set_], dtype=dtype)        # [entries][nfeat] (bcast: [entries][1])
        for lv in range(desc["nlv"]):
            for p in range(3):
                W, H, Ln = plane_dims(case["grid"])[p]
                Cn = desc["C"][p]
                feats = [f for f, (_, l, pp, _, _) in enumerate(fmap) if l == lv and pp == p]
                assert [fmap[f][3] for f in feats] == list(range(Cn))
                dq = dq_all[erow][:, [0] * Cn] if desc["bcast"] else dq_all[erow][:, feats]
                ax, ay, al = AXES[p]
                Ws, Hs, Ls = sub(W, lv), sub(H, lv), sub(Ln, lv)
                ix, wx0, wx1, okx0, okx1 = tap1d(xs[idx, ax], Ws)
                iy, wy0, wy1, oky0, oky1 = tap1d(xs[idx, ay], Hs)
                il, wl0, wl1, okl0, okl1 = tap1d(xs[idx, al], Ls)
                plane = np.asarray(case["planes"][set_][p], dtype=dtype)[:: 1 << lv, :: 1 << lv]
                line = np.asarray(case["lines"][set_][p], dtype=dtype)[:: 1 << lv]
                assert plane.shape[:2] == (Hs, Ws) and line.shape[0] == Ls

                def tapv(arr2, yy, xx, ok):
                    v = arr2[np.clip(yy, 0, Hs - 1), np.clip(xx, 0, Ws - 1)]
                    return np.where(ok[:, None], v, 0)

                taps = [(iy, ix, oky0 & okx0, wx0 * wy0), (iy, ix + 1, oky0 & okx1, wx1 * wy0),
                        (iy + 1, ix, oky1 & okx0, wx0 * wy1), (iy + 1, ix + 1, oky1 & okx1, wx1 * wy1)]
                v = [tapv(plane, yy, xx, ok) for yy, xx, ok, _ in taps]
                a0 = np.where(okl0[:, None], line[np.clip(il, 0, Ls - 1)], 0)
                a1 = np.where(okl1[:, None], line[np.clip(il + 1, 0, Ls - 1)], 0)
                w = [t[3].astype(dtype)[:, None] for t in taps]
                wx0_, wx1_, wy0_, wy1_ = (a.astype(dtype)[:, None] for a in (wx0, wx1, wy0, wy1))
                wl0_, wl1_ = wl0.astype(dtype)[:, None], wl1.astype(dtype)[:, None]
                pv = v[0] * w[0] + v[1] * w[1] + v[2] * w[2] + v[3] * w[3]
                lvv = a0 * wl0_ + a1 * wl1_
                dp, dl = dq * lvv, dq * pv
                comp = np.arange(Cn)[None, :]
                samp = np.broadcast_to(idx[:, None], dq.shape)
                for (yy, xx, ok, _), wk in zip(taps, w):
                    flat = ((np.clip(yy, 0, Hs - 1)[:, None] << lv) * W + (np.clip(xx, 0, Ws - 1)[:, None] << lv)) * Cn + comp
                    val = np.where(ok[:, None], dp * wk, 0)
                    emit(("plane", set_, p), flat.ravel(), val.ravel(), samp.ravel())
                for ll, ok, wk in ((il, okl0, wl0_), (il + 1, okl1, wl1_)):
                    flat = (np.clip(ll, 0, Ls - 1)[:, None] << lv) * Cn + comp
                    val = np.where(ok[:, None], dl * wk, 0)
                    emit(("line", set_, p), flat.ravel(), val.ravel(), samp.ravel())
                half = dtype(0.5)
                gcx = half * dtype(Ws - 1) * dp * ((v[1] - v[0]) * wy0_ + (v[3] - v[2]) * wy1_)
                gcy = half * dtype(Hs - 1) * dp * ((v[2] - v[0]) * wx0_ + (v[3] - v[1]) * wx1_)
                gcl = half * dtype(Ls - 1) * dl * (a1 - a0)
                for axis, gval in ((ax, gcx), (ay, gcy), (al, gcl)):
                    flat = np.broadcast_to(idx[:, None] * 3 + axis, gval.shape)
                    emit("dw", flat.ravel(), gval.ravel(), samp.ravel())
    res = {}
    for key, parts in out.items():
        res[key] = tuple(np.concatenate([p[i] for p in parts]) for i in range(3))
    return res


def shapes(case):
    desc = case["desc"]
    ns = case["N"] * case["S"]
    sh = {}
    for set_ in range(desc["nsets"]):
        for p, (W, H, Ln) in enumerate(plane_dims(case["grid"])):
            sh[("plane", set_, p)] = (H, W, desc["C"][p])
            sh[("line", set_, p)] = (Ln, desc["C"][p])
    sh["dxw"] = (ns, 3)
    sh["g_xyz"] = (ns, 3)
    return sh


def _targets(case, tm, mode):
    """route the "dw" stream to the outputs of this kind and mode: (output name, flat, value, sample, scale, overwrite)"""
    desc = case["desc"]
    routes = [(k, f, v, s, 1.0, False) for k, (f, v, s) in tm.items() if k != "dw"]
    f, v, s = tm.get("dw", (np.zeros(0, np.int64), np.zeros(0), np.zeros(0, np.int64)))
    dmode = desc["dxw_ray"] if mode == "ray" else desc["dxw_sorted"]
    if dmode:
        routes.append(("dxw", f, v, s, 1.0, dmode == 1))
    if desc["g_xyz"]:
        inv = np.asarray(case["box_inv"], dtype=np.float64)[f % 3] if len(f) else np.zeros(0)
        routes.append(("g_xyz", f, v, s, inv, False))
    return routes


class HeadroomError(AssertionError):
    pass


def reference(case, mode="ray", how="exact", prefill=None, perm_seed=None, tm=None):
    """how: "exact" (int64 fixed point; asserts the headroom), "f64", "seq32" (float32, terms added in sample order).
    perm_seed (seq32): the terms of every output are added in a random order instead; tm: terms(case, dtype) computed before.
    Returns ({output: array}, {output: sum |terms|}); outputs that the kind does not write keep their pre-fill."""
    desc = case["desc"]
    dtype = f32 if how == "seq32" else np.float64
    tm = terms(case, dtype) if tm is None else tm
    sh = shapes(case)
    pre = {k: np.zeros(s) for k, s in sh.items()} if prefill is None else prefill
    res, mag = {}, {}
    written = np.zeros(sh["dxw"][0], dtype=bool)
    written[entries(case)[0]] = True
    routes = {r[0]: r for r in _targets(case, tm, mode)}
    for key, shp in sh.items():
        base = np.asarray(pre[key], dtype=np.float64).reshape(-1).copy()
        if key not in routes:
            res[key], mag[key] = base.reshape(shp), np.abs(base).reshape(shp)
            continue
        _, flat, val, samp, scale, overwrite = routes[key]
        if overwrite:
            base.reshape(shp)[written] = 0.0
        if how == "exact":
            tv0 = np.asarray(val, dtype=np.float64) * scale
            # q: the fractional bits this output really needs (at most Q): every term and the pre-fill are multiples of 2^-q, so
            # every partial sum is one too, and below 2^24 2^-q in magnitude it is exact in fp32
            for q in range(Q + 1):
                tv, b = tv0 * 2.0 ** q, base * 2.0 ** q
                if (tv == np.rint(tv)).all() and (b == np.rint(b)).all():
                    break
            else:
                raise HeadroomError(f"{key}: a term is not a multiple of 2^-{Q}")
            acc = np.rint(b).astype(np.int64)
            ab = np.abs(acc)
            np.add.at(acc, flat, np.rint(tv).astype(np.int64))
            np.add.at(ab, flat, np.abs(np.rint(tv)).astype(np.int64))
            if ab.size and ab.max() >= 2 ** 24:
                raise HeadroomError(f"{key}: sum |terms| 2^{q} = {ab.max()} >= 2^24: a partial sum may round in fp32")
            res[key], mag[key] = (acc.astype(np.float64) / 2.0 ** q).reshape(shp), (ab.astype(np.float64) / 2.0 ** q).reshape(shp)
        else:
            order = np.argsort(samp, kind="stable") if perm_seed is None else np.random.default_rng(perm_seed).permutation(len(samp))
            acc = base.astype(dtype)
            tv = (np.asarray(val, dtype=dtype) * np.asarray(scale, dtype=dtype))[order]
            np.add.at(acc, flat[order], tv)          # unbuffered, in order, in acc's dtype
            ab = np.abs(base)
            np.add.at(ab, flat, np.abs(np.asarray(val, dtype=np.float64) * scale))
            res[key], mag[key] = acc.astype(np.float64).reshape(shp), ab.reshape(shp)
    return res, mag


# ---- keys, sort, counts --------------------------------------------------------------------------------------------------------
def reference_keys(case):
    """(keys [3 nent], sorted keys, order, counts [3]) of the sorted forms: key = plane << kb | cell, cell = iy (W + 3) + ix of the
    level-0 tap index clamped to [-2, L] + 2; an entry that is not live, or that has no in-range tap at any level on one of the two
    axes, takes the drop code (all ones)."""
    desc = case["desc"]
    kb, ns = desc["kb"], case["N"] * case["S"]
    xs = normalise(case)
    if desc["list"]:
        ids = np.asarray(case["list"][: case["count"]], dtype=np.int64)
        live = np.ones(len(ids), dtype=bool)
    else:
        ids = np.arange(ns)
        live = (np.asarray(case["valid"]).reshape(-1) != 0) & case["sm_live"].reshape(-1)
    nent = len(ids)
    keys = np.zeros(3 * nent, dtype=np.uint32)
    for p, (W, H, _) in enumerate(plane_dims(case["grid"])):
        ax, ay, _ = AXES[p]

        def axis(c, Ln):
            t = [tap1d(c, sub(Ln, lv)) for lv in range(3)]
            anyok = np.zeros(len(c), dtype=bool)
            for tt in t:
                anyok |= tt[3] | tt[4]
            return np.minimum(np.maximum(t[0][0], -2), Ln) + 2, anyok
        ixc, okx = axis(xs[ids, ax], W)
        iyc, oky = axis(xs[ids, ay], H)
        cell = np.where(live & okx & oky, iyc * desc["wk"][p] + ixc, (1 << kb) - 1)
        assert desc["wk"][p] == W + 3 and cell.max(initial=0) < (1 << kb)
        keys[p * nent:(p + 1) * nent] = (p << kb) | cell.astype(np.uint32)
    order = np.argsort(keys, kind="stable").astype(np.uint32)
    ks = keys[order]
    counts = [int(((ks >> kb) == p).sum() - (ks == ((p << kb) | ((1 << kb) - 1))).sum()) for p in range(3)]
    return keys, ks, order, counts


def reference_sort(keys, bits, n_sorted=None):
    """stable ascending sort on the low `bits` bits of the first n_sorted keys: (sorted keys, order)"""
    k = np.asarray(keys, dtype=np.uint32)[: len(keys) if n_sorted is None else n_sorted]
    digit = k & np.uint32(0xffffffff if bits >= 32 else (1 << bits) - 1)
    order = np.argsort(digit, kind="stable").astype(np.uint32)
    return k[order], order


# ---- cases -------------------------------------------------------------------------------------------------------------------
def make_case(desc, grid, N, S, coords, rng, valid=None, list_=None, set_mask=None, flat=0, mag=2, density=1.0, dense=False,
              box_lo=(-2.0, -4.0, -1.0), box_inv=(0.5, 0.25, 1.0), sm_dead=None, nonzero=False):
    """factor values and d(features): integers in [-mag, mag] (dense: normal), a fraction `density` of the d(feature) rows
    non-zero (nonzero: no zero among the integers at all).  coords: [N S][3] NORMALISED coordinates; the static kinds receive xyz = (c + 1) / inv + lo (exact for dyadic c)."""
    ns = N * S
    nsets = desc["nsets"]
    if dense:
        draw = lambda *s: rng.standard_normal(s)
    elif nonzero:      # no value is zero: no factor value or d(feature) can hide a dropped or doubled tap
        draw = lambda *s: (rng.integers(1, mag + 1, s) * rng.choice([-1, 1], s)).astype(np.float64)
    else:
        draw = lambda *s: rng.integers(-mag, mag + 1, s).astype(np.float64)
    case = dict(desc=desc, grid=list(grid), N=N, S=S, flat=flat, set_mask=(3 if nsets == 2 else 1) if set_mask is None else set_mask)
    case["planes"] = [[draw(H, W, desc["C"][p]) for p, (W, H, _) in enumerate(plane_dims(grid))] for _ in range(nsets)]
    case["lines"] = [[draw(Ln, desc["C"][p]) for p, (_, _, Ln) in enumerate(plane_dims(grid))] for _ in range(nsets)]
    c = np.asarray(coords, dtype=f32).reshape(ns, 3)
    case["box_lo"], case["box_inv"] = list(box_lo), list(box_inv)
    if desc["xw"]:
        case["coords"] = c
    else:
        with np.errstate(over="ignore"):
            case["coords"] = ((c.astype(np.float64) + 1.0) / np.asarray(box_inv) + np.asarray(box_lo)).astype(f32)
    case["valid"] = np.ones(ns, dtype=np.uint8) if valid is None else np.asarray(valid, dtype=np.uint8).reshape(ns)
    sm_live = np.ones(ns, dtype=bool)
    if sm_dead is not None:
        sm_live[np.asarray(sm_dead)] = False
    case["sm_live"] = sm_live
    if desc["list"]:
        case["list"] = np.arange(ns, dtype=np.int32) if list_ is None else np.asarray(list_, dtype=np.int32)
        case["count"] = len(case["list"])
        nent = case["count"]
    else:
        nent = ns
    nf = 1 if desc["bcast"] else desc["nfeat"]
    case["dq"] = []
    for _ in range(nsets):
        dq = draw(nent, nf)
        if density < 1.0:
            dq *= (rng.random((nent, 1)) < density)
        if not desc["list"]:
            dq[~sm_live] = 0.0          # a sample whose head gradients are zero has zero d(features), as in the product
        case["dq"].append(dq)
    return case


def layout_rows(case):
    """the d(feature) rows [tiles][stride][32] float32 of the ray modes (and the liveness rows of the sorted density form)"""
    desc = case["desc"]
    N, S, ns = case["N"], case["S"], case["N"] * case["S"]
    tpr = (S + 31) // 32
    if desc["list"] or case["flat"]:
        nent = case["count"] if desc["list"] else ns
        tiles = (ns + 31) // 32
        e = np.arange(nent)
        tile, slot = e // 32, e % 32
    else:
        tiles = N * tpr
        e = np.arange(ns)
        tile, slot = (e // S) * tpr + (e % S) // 32, (e % S) % 32
    rows = np.zeros((tiles, desc["stride"], 32), dtype=f32)
    fmap = feature_map(desc)
    for set_ in range(desc["nsets"]):
        dq = case["dq"][set_]
        if desc["bcast"]:
            rows[tile, desc["row0"][set_], slot] = dq[:, 0]
        else:
            for f, (row, *_rest) in enumerate(fmap):
                rows[tile, desc["row0"][set_] + row, slot] = dq[:, f]
    for r in desc["live_rows"]:
        if r >= 0:
            rows[tile, r, slot] = case["sm_live"].astype(f32)
    return rows


def layout_recs(case):
    """the sample-major records [N S][rec_floats] float32 of the sorted modes"""
    desc = case["desc"]
    ns = case["N"] * case["S"]
    recs = np.zeros((ns, desc["rec_floats"]), dtype=f32)
    fmap = feature_map(desc)
    for set_ in range(desc["nsets"]):
        dq = case["dq"][set_]
        for f, (_, _, _, _, slot) in enumerate(fmap):
            recs[: dq.shape[0], set_ * desc["set_floats"] + slot] = dq[:, f]
    return recs


def dyadic_coords(rng, grid, n, lo=-2, hi=2):
    """c = -1 + m / 2^k per axis for a 2^k + 1 grid, m in [lo, 2^(k+1) + hi]: weights are multiples of 1/2 (level 0) .. 1/8"""
    out = np.zeros((n, 3), dtype=f32)
    for a, g in enumerate(grid):
        k = int(np.log2(g - 1))
        assert (1 << k) + 1 == g, "the exact cases need 2^k + 1 grids"
        out[:, a] = -1.0 + rng.integers(lo, (2 << k) + hi + 1, n) / float(1 << k)
    return out


def error_metric(res, g64, mag):
    """per output: e = max |g - g64| / sum |terms| over the elements that receive a term"""
    out = {}
    for k in g64:
        nz = mag[k] > 0
        if nz.any():
            out[k] = float((np.abs(res[k] - g64[k])[nz] / mag[k][nz]).max())
    return out


def dense_case(desc, grid, seed=11, N=40, S=48):
    """the dense class: normal values, uniform coordinates in [-1.05, 1.05], an unsorted list of 1500 for the appearance kinds"""
    rng = np.random.default_rng(seed)
    coords = rng.uniform(-1.05, 1.05, (N * S, 3))
    kw = dict(list_=rng.permutation(N * S)[:1500]) if desc["list"] else {}
    return make_case(desc, grid, N, S, coords, rng, dense=True, box_lo=(-1.5, -1.7, -1.0), box_inv=(2 / 3.0, 2 / 3.4, 1.0),
                     flat=1 if desc["flat"] else 0, **kw)
