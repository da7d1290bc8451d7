"""Float64 references, seeded generators and derived bounds for the data gradients of two links of the backward-data chain, shared by
test_warp_primitives_cpu.py, test_gpu_warp_primitives.py and the exact checks of test_gpu_warp_dw_fused.py / test_gpu_scene_flow_fused.py.
No GPU.
  * the warp MLP's tile on flat tiles behind rdrf_selftest_warp_bwd (k_dyn_warp_bwd_dw, and in the tools build its partner
    k_dyn_density_bwd<1, false, true>): g_xyz, the small-layer dz rows 0..2 (dd) and d(tout) per ray;
  * the scene-flow backward behind rdrf_scene_flow_bwd (k_scene_flow_bwd_dw, partner k_scene_flow_bwd): g_pts.
Out of scope, because rdrf_selftest_warp_bwd does not reach them: the feature-mode warp tile (k_dyn_density_bwd<1, true>, in_norm)
and the wave-per-ray warp tile.

Every reference takes the float32 inputs the kernel gets, widens them to float64 and returns, per output, the value and an absolute
bound  k U cond (+ what the bounds of its inputs contribute), U = 2^-24 the unit roundoff of one fp32 operation, cond the sum of the
absolute values of the terms added and k the count of the kernel's rounded operations on the way.  The counts are first order; every
bound is multiplied by SECOND = 1 + 2^-12, which covers the products of two roundings (k U < 2^-12 for every k here), and gets TINY =
2^-126 where cond > 0 (a term below the smallest normal number may be flushed).  An output whose cond is 0 has the bound 0: it must be
exactly 0.  No constant was tuned against the kernels.

Layouts are not written down here.  The saved row of every weight column and the dz rows come from rdrf_selftest_dw_describe (the
DENSITY and SCENE_FLOW plans: block row0 + i holds the weight column cols[i]), the d(X0) and small-layer dz rows and the row counts
from rdrf_selftest_heads_describe.  What a weight COLUMN means is the model's definition of the layer's input, [x 3 | sin(2^f x_d),
d-major | cos likewise | ...] (tests/_gather_prim.py encodings_reference holds the forward encoding to the same order).

Warp, per sample, inv = fl32(2 / fl32(hi - lo)) per axis:
    dd  = dxw inv + g_xyz_prime            a product and a sum: k = 2, cond = |dxw inv| + |g_xyz_prime|   (rows SM + 0..2, 0 past N S)
    dz4 = [H4 > 0] W5^T dd                 VALU, three products and two sums: k = 3
    dz3 = [H3 > 0] W4^T dz4                mfma_seg_b3<2, 32>: _heads_prim.b3_pair_bound of these inputs (2 e_seq32 + ONE_HOT_BOUND)
    dX0 = heads' rows + W3[:, X0]^T dz3    mfma_seg_b3_pair<2, 1, 32> on an accumulator that starts at the heads' value: the same
    dT  = W3[:, 63:93]^T dz3               bound with the heads' value as one more term of cond, and U cond for that addend
    e_d = dX0[x_d] + sum_f 2^f (dS c - dC s)    per pair two products and a difference (k = 2, uncontracted; a contraction saves
                                           one), ldexp exact; 11 terms per axis over the two lane halves and their combine: 10 sums
    dn  = dxn + (e + dxw)                  k = 2
    g_xyz += dn inv + g_xyz_prime          a product, a sum and the addition onto the pre-fill: k = 3
    d(tout)[ray] = sum of dT over the ray's samples: five butterfly stages per tile record (k = 5); the records of a ray that spans
    tiles are added in float64 by the test (ray_dtout), as the comparison reads them.
Scene flow:
    dz4 = [H4 > 0] W3^T [g_f, g_b]         six fma: k = 6
    dz2, dz0, dX                           mfma_seg in fp32 over 64 inputs: chains of 64, k = 64 each
    e_d = dX[x_d] + sum_{f<4} 2^f (dS c - dC s)   k = 2 per pair, 5 terms per axis: 4 sums;  the time pairs (12 ..) add nothing
    g_pts += e inv                         a product and the addition onto the pre-fill: k = 2
eval32 of each reference is the same equations in numpy float32, every product and sum rounded, the terms added one after the other;
test_warp_primitives_cpu.py shows that it meets every bound and that each mutation of it (MUTATIONS) does not."""
import numpy as np

import _dw_prim as DW
import _heads_prim as HP
import _mlp_prim as MP

f32, f64 = np.float32, np.float64
U = 2.0 ** -24
TINY = 2.0 ** -126
SECOND = 1.0 + 2.0 ** -12
NAN = HP.NAN
ratio = HP.ratio

BOX_UNIT = np.array([[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]], dtype=f32)
BOX_POW2 = np.array([[-2.0, -1.0, -4.0], [2.0, 1.0, 4.0]], dtype=f32)          # inv = (0.5, 1, 0.25): exact, all different
BOX_ODD = np.array([[-1.5, -1.67, -1.0], [1.5, 1.67, 1.0]], dtype=f32)         # no power of two: the scene-flow harness's own box
GATES = np.array([0.0, -0.0, 2.0 ** -126, -2.0 ** -126, 1.0, -1.0], dtype=f32)

WARP_EXACT = [(n, 1) for n in (1, 31, 32, 33, 129, 257)] + [(3, 45), (23, 45)]
WARP_DENSE = [(200, 41), (26, 45)]      # 257 tiles (the dense shape of test_gpu_warp_dw_fused.py) and 37, the last one partly empty
SF_EXACT = [1, 31, 32, 33, 160, 257]
SF_DENSE = 257 * 32 - 5
MUTATIONS = ("swap_inv", "no_inv_dd", "no_inv_g", "no_dxn", "swap_sc", "freq_off", "pair_shift", "no_identity", "time_pairs")
WARP_MUTATIONS = MUTATIONS[:-1]
SF_MUTATIONS = ("swap_inv", "no_inv_g", "swap_sc", "freq_off", "pair_shift", "no_identity", "time_pairs")


def box_inv(box):
    """box.inv as make_box forms it: 2 / (hi - lo), the difference and the quotient rounded to float32"""
    box = np.asarray(box, dtype=f32)
    return (f32(2.0) / (box[1] - box[0]).astype(f32)).astype(f32)


# ---- layouts from the library ------------------------------------------------------------------------------------------------
def _job(desc, off):
    js = [j for j in desc["jobs"] if j["w_off"] == off]
    assert len(js) == 1, off
    return js[0]


def _row_of_col(job):
    """saved row of every weight column of the job"""
    row = np.full(job["in_dim"], -1, dtype=np.int64)
    for row0, cols in job["blocks"]:
        ok = cols >= 0
        row[cols[ok]] = row0 + np.nonzero(ok)[0]
    assert (row >= 0).all()
    return row


_LAY = {}


def warp_layout(L):
    """rows / grows per tile, DX0 / SM: first d(X0) / small-layer dz row, in3 [93] / H3 [64] / H4 [64]: saved row of every column of
    layer3 / layer4 / layer5, x0_row0: first row of the X0 block (d(X0) row DX0 + r belongs to saved row x0_row0 + r)"""
    if "warp" not in _LAY:
        d = DW.describe(L, "DENSITY", 0)
        hd = HP.heads_describe(L, 0, 1, 1)
        j3, j4, j5 = (_job(d, getattr(L.RdrfDynamicParams, n).offset) for n in ("l3w", "l4w", "l5w"))
        assert (j3["in_dim"], j4["in_dim"], j5["in_dim"], j5["out_dim"]) == (93, 64, 64, 3) and j5["A_row0"] + j5["out_row0"] == hd["sm"]
        in3 = _row_of_col(j3)
        x0_row0 = min(r for r, cols in j3["blocks"] if 0 <= cols.max() < 63)
        assert 0 <= in3[:63].min() - x0_row0 and in3[:63].max() - x0_row0 < 64
        _LAY["warp"] = dict(rows=hd["rows"], grows=hd["grows"], DX0=hd["dx0"], SM=hd["sm"], in3=in3, H3=_row_of_col(j4), H4=_row_of_col(j5),
                            x0_row0=x0_row0)
    return _LAY["warp"]


def sf_layout(L):
    """rows per tile, X [36] / H0 / H2 / H4 [64]: saved row of every column of scene_flow_mlp.{0, 2, 4, 6}.weight"""
    if "sf" not in _LAY:
        d = DW.describe(L, "SCENE_FLOW", 0)
        base = L.RdrfDynamicParams.sfw.offset
        js = [_job(d, base + 8 * i) for i in range(4)]
        assert [j["in_dim"] for j in js] == [36, 64, 64, 64] and js[3]["out_dim"] == 6
        _LAY["sf"] = dict(rows=d["regions"][0][1], X=_row_of_col(js[0]), H0=_row_of_col(js[1]), H2=_row_of_col(js[2]), H4=_row_of_col(js[3]))
    return _LAY["sf"]


def samples(arr, n):
    """[T][R][32] rows -> [n][R]: sample i = 32 tile + lane"""
    T, R = arr.shape[0], arr.shape[1]
    return arr.transpose(0, 2, 1).reshape(T * 32, R)[:n]


def put_rows(arr, rows, vals):
    """vals [n][len(rows)] into the rows `rows` of arr [T][R][32], the slots past n untouched"""
    T, n = arr.shape[0], vals.shape[0]
    full = arr[:, rows, :].transpose(0, 2, 1).reshape(T * 32, len(rows)).copy()
    full[:n] = vals
    arr[:, rows, :] = full.reshape(T, 32, len(rows)).transpose(0, 2, 1)


# ---- the encoding backward, both fields -------------------------------------------------------------------------------------------
def pe_backward(X, dX, bX, F, sums):
    """X, dX, bX [n][3 + 6 F ..] in COLUMN order [x 3 | sin d-major | cos]: -> e [n][3], its cond and its bound (module docstring);
    sums: the rounded additions on an axis"""
    n = X.shape[0]
    e, cond, b = dX[:, :3].copy(), np.abs(dX[:, :3]), bX[:, :3].copy()
    for j in range(3 * F):
        d, f = divmod(j, F)
        s, c, dS, dC = X[:, 3 + j], X[:, 3 + 3 * F + j], dX[:, 3 + j], dX[:, 3 + 3 * F + j]
        w = 2.0 ** f
        e[:, d] += w * (dS * c - dC * s)
        t = w * (np.abs(dS * c) + np.abs(dC * s))
        cond[:, d] += t
        b[:, d] += w * (bX[:, 3 + j] * np.abs(c) + bX[:, 3 + 3 * F + j] * np.abs(s)) + 2 * U * t
    assert e.shape == (n, 3)
    return e, cond, b + sums * U * cond


def pe_backward32(X, dX, F, mut=(), time_cols=None):
    """the same in float32, uncontracted, the pairs added one after the other; mut: the wrong kernels of MUTATIONS"""
    e = np.zeros((X.shape[0], 3), dtype=f32) if "no_identity" in mut else dX[:, :3].astype(f32).copy()
    for j in range(3 * F):
        s, c, dS, dC = X[:, 3 + j], X[:, 3 + 3 * F + j], dX[:, 3 + j], dX[:, 3 + 3 * F + j]
        if "swap_sc" in mut:
            s, c = c, s
        d, f = divmod((j + 1) % (3 * F) if "pair_shift" in mut else j, F)
        dq = np.ldexp(((dS * c).astype(f32) - (dC * s).astype(f32)).astype(f32), f + 1 if "freq_off" in mut else f).astype(f32)
        e[:, d] = (e[:, d] + dq).astype(f32)
    if "time_pairs" in mut and time_cols is not None:   # pairs 12 .. land on axis (pair >> 2) & 3 = 3 -> wrapped to 0
        for f, (cs, cc) in enumerate(time_cols):
            dq = np.ldexp(((dX[:, cs] * X[:, cc]).astype(f32) - (dX[:, cc] * X[:, cs]).astype(f32)).astype(f32), f).astype(f32)
            e[:, 0] = (e[:, 0] + dq).astype(f32)
    assert e.dtype == f32
    return e


def _finish(bound, cond):
    return np.where(cond > 0, SECOND * bound + TINY, 0.0)


# ---- warp: inputs ------------------------------------------------------------------------------------------------------------------
def _int_weights(rng, shapes):
    W = {}
    for k, (out, inn) in shapes.items():
        w = np.zeros((out, inn), dtype=f32)
        for c in range(inn):
            w[rng.choice(out, size=2, replace=False), c] = rng.choice([-1.0, 1.0], size=2)
        W[k] = w
    return W


WARP_SHAPES = {"l3": (64, 93), "l4": (64, 64), "l5": (3, 64)}
SF_SHAPES = [(64, 36), (64, 64), (64, 64), (6, 64)]


def warp_case(lay, kind, N, S, seed=0, box=BOX_POW2, enc="normal", gp=True):
    """kind 'exact': small integers (weights in {-1, 0, 1}, two per input column; rows in [-2, 2]; gradients in {-1, 0, 1}, dxn in
    [-2, 2]; g_xyz pre-filled with integers in [0, 4]) on a box whose inv are powers of two -- the generator asserts that the largest
    sum of absolute terms of every output, in units of the output's quantum, stays below 2^24, so that no order of accumulation and
    no contraction can change a bit.  'dense': normal rows and weights; enc 'sincos': the X0 rows are the real sin / cos of a drawn xn,
    'normal': independent normals (the kernel reads the saved rows and owes nothing to s^2 + c^2 = 1).  'gate_edges': dense, the H3 / H4
    rows drawn from GATES."""
    n = N * S
    T = (n + 31) // 32
    rng = np.random.default_rng([43, ("exact", "dense", "gate_edges").index(kind), seed, N, S])
    if kind == "exact":
        act = rng.integers(-2, 3, size=(T, lay["rows"], 32)).astype(f32)
        grw = rng.integers(-2, 3, size=(T, lay["grows"], 32)).astype(f32)
        W = _int_weights(rng, WARP_SHAPES)
        dxw, dxn, g = (rng.integers(-1, 2, size=(n, 3)).astype(f32), rng.integers(-2, 3, size=(n, 3)).astype(f32),
                       rng.integers(-1, 2, size=(n, 3)).astype(f32))
        pre = rng.integers(0, 5, size=(n, 3)).astype(f32)
    else:
        act = rng.standard_normal((T, lay["rows"], 32), dtype=f32)
        grw = rng.standard_normal((T, lay["grows"], 32), dtype=f32)
        W = {k: (rng.standard_normal(s, dtype=f32) / f32(np.sqrt(s[1]))).astype(f32) for k, s in WARP_SHAPES.items()}
        dxw, dxn, g = (rng.standard_normal((n, 3), dtype=f32) for _ in range(3))
        pre = rng.integers(-3, 4, size=(n, 3)).astype(f32)
        if enc == "sincos":
            xn = rng.uniform(-1.0, 1.0, size=(n, 3)).astype(f32)
            q = np.stack([np.ldexp(xn[:, d], f) for d in range(3) for f in range(10)], -1).astype(f32).astype(f64)
            put_rows(act, lay["in3"][:63], np.concatenate([xn, np.sin(q).astype(f32), np.cos(q).astype(f32)], -1))
        if kind == "gate_edges":
            for key in ("H3", "H4"):
                put_rows(act, lay[key], GATES[rng.integers(0, len(GATES), size=(n, 64))])
    c = dict(kind=kind, N=N, S=S, act=act, grw=grw, W=W, dxw=dxw, dxn=dxn, gp=g if gp else None, pre=pre, box=np.asarray(box, dtype=f32))
    if kind == "exact":
        c["max_quanta"] = warp_exact_guard(c, lay)
    return c


def warp_exact_guard(c, lay):
    """largest sum of absolute terms of any output or intermediate of an integer case, in units of its quantum (every input is an
    integer and every inv a power of two 2^-a, a <= 2: dd and all that follows it are multiples of 2^-2, g_xyz of 2^-4); the factor 2^9
    of the encoding is in cond.  Below 2^24 every partial sum is a float32 number: any order and any contraction give the same bits."""
    inv = box_inv(c["box"]).astype(f64)
    assert all(v in (0.25, 0.5, 1.0) for v in inv), inv
    r = warp_reference(c, lay)
    worst = max(float(r["cond"][k].max(initial=0.0)) * q for k, q in (("dd", 4), ("dz4", 4), ("dz3", 4), ("dX0", 4), ("dT", 4), ("e", 4),
                                                                        ("dn", 4), ("g_xyz", 16), ("dtout", 4)))
    assert worst < 2 ** 24, worst
    return worst


# ---- warp: reference ---------------------------------------------------------------------------------------------------------------
def _warp_inputs(c, lay, dtype):
    n = c["N"] * c["S"]
    a, g = samples(c["act"], n).astype(dtype), samples(c["grw"], n).astype(dtype)
    in3 = lay["in3"]
    X0 = a[:, in3[:63]]
    hX = g[:, lay["DX0"] + in3[:63] - lay["x0_row0"]]
    W = {k: v.astype(dtype) for k, v in c["W"].items()}
    gp = np.zeros((n, 3), dtype=dtype) if c["gp"] is None else c["gp"].astype(dtype)
    pre = np.zeros((n, 3), dtype=dtype) if c.get("pre") is None else c["pre"].astype(dtype)
    return n, X0, hX, a[:, lay["H3"]] > 0, a[:, lay["H4"]] > 0, W, c["dxw"].astype(dtype), c["dxn"].astype(dtype), gp, pre


def warp_reference(c, lay):
    """-> {'dd': (value [T 32][3], bound), 'g_xyz': ([n][3], bound), 'dtout': ([N][30], bound), 'cond': {name: cond}}; plus the
    intermediates 'dz4', 'dz3', 'dX0' (column order, 63), 'dT', 'e', 'dn' as (value, bound)"""
    n, X0, hX, G3, G4, W, dxw, dxn, gp, pre = _warp_inputs(c, lay, f64)
    inv = box_inv(c["box"]).astype(f64)[None, :]
    T = c["act"].shape[0]
    cond = {}
    dd = dxw * inv + gp
    cond["dd"] = np.abs(dxw * inv) + np.abs(gp)
    bdd = 2 * U * cond["dd"]
    A5, A4, A3 = np.abs(W["l5"]), np.abs(W["l4"]), np.abs(W["l3"])
    dz4 = np.where(G4, dd @ W["l5"], 0.0)
    cond["dz4"] = np.where(G4, np.abs(dd) @ A5, 0.0)
    bdz4 = np.where(G4, bdd @ A5 + 3 * U * cond["dz4"], 0.0)
    rel4 = HP.b3_pair_bound(dz4.astype(f32), c["W"]["l4"].T)
    dz3 = np.where(G3, dz4 @ W["l4"], 0.0)
    cond["dz3"] = np.where(G3, np.abs(dz4) @ A4, 0.0)
    bdz3 = np.where(G3, bdz4 @ A4 + rel4 * cond["dz3"], 0.0)
    rel3 = HP.b3_pair_bound(dz3.astype(f32), c["W"]["l3"].T)
    dX = hX + dz3 @ W["l3"][:, :63]
    cond["dX0"] = np.abs(hX) + np.abs(dz3) @ A3[:, :63]
    bdX = bdz3 @ A3[:, :63] + (rel3 + U) * cond["dX0"]
    dT = dz3 @ W["l3"][:, 63:]
    cond["dT"] = np.abs(dz3) @ A3[:, 63:]
    bdT = bdz3 @ A3[:, 63:] + rel3 * cond["dT"]
    e, cond["e"], be = pe_backward(X0, dX, bdX, 10, 10)
    dn = dxn + e + dxw
    cond["dn"] = np.abs(dxn) + cond["e"] + np.abs(dxw)
    bdn = be + 2 * U * cond["dn"]
    gx = pre + dn * inv + gp
    cond["g_xyz"] = np.abs(pre) + cond["dn"] * inv + np.abs(gp)
    bgx = bdn * inv + 3 * U * cond["g_xyz"]
    dt = dT.reshape(c["N"], c["S"], 30).sum(1)
    cond["dtout"] = np.abs(dT).reshape(c["N"], c["S"], 30).sum(1)
    bdt = bdT.reshape(c["N"], c["S"], 30).sum(1) + 5 * U * cond["dtout"]

    def pad(v):
        full = np.zeros((T * 32, 3))
        full[:n] = v
        return full

    fin = lambda b, k: _finish(b, cond[k])
    return {"dd": (pad(dd), pad(fin(bdd, "dd"))), "g_xyz": (gx, fin(bgx, "g_xyz")), "dtout": (dt, fin(bdt, "dtout")), "cond": cond,
            "dz4": (dz4, fin(bdz4, "dz4")), "dz3": (dz3, fin(bdz3, "dz3")), "dX0": (dX, fin(bdX, "dX0")), "dT": (dT, fin(bdT, "dT")),
            "e": (e, fin(be, "e")), "dn": (dn, fin(bdn, "dn"))}


def _mut_inv(inv, mut):
    return inv[[1, 0, 2]] if "swap_inv" in mut else inv


def warp_eval32(c, lay, mut=()):
    """-> {'dd' [T 32][3], 'g_xyz' [n][3], 'dtout' [N][30]} in float32 (module docstring); mut: wrong kernels (MUTATIONS)"""
    n, X0, hX, G3, G4, W, dxw, dxn, gp, pre = _warp_inputs(c, lay, f32)
    inv = _mut_inv(box_inv(c["box"]), mut)[None, :]
    one = np.ones_like(inv)
    zero = f32(0.0)
    dd = ((dxw * (one if "no_inv_dd" in mut else inv)).astype(f32) + gp).astype(f32)
    dz4 = np.where(G4, MP.seq32(dd, np.ascontiguousarray(W["l5"].T)), zero)
    dz3 = np.where(G3, MP.seq32(dz4, np.ascontiguousarray(W["l4"].T)), zero)
    dX = (hX + MP.seq32(dz3, np.ascontiguousarray(W["l3"][:, :63].T))).astype(f32)
    dT = MP.seq32(dz3, np.ascontiguousarray(W["l3"][:, 63:].T))
    e = pe_backward32(X0, dX, 10, mut)
    dn = ((zero * dxn if "no_dxn" in mut else dxn) + (e + dxw).astype(f32)).astype(f32)
    gx = (pre + ((dn * (one if "no_inv_g" in mut else inv)).astype(f32) + gp).astype(f32)).astype(f32)
    dt = np.zeros((c["N"], 30), dtype=f32)
    per = dT.reshape(c["N"], c["S"], 30)
    for j in range(c["S"]):
        dt = (dt + per[:, j]).astype(f32)
    full = np.zeros((c["act"].shape[0] * 32, 3), dtype=f32)
    full[:n] = dd
    assert full.dtype == gx.dtype == dt.dtype == f32
    return {"dd": full, "g_xyz": gx, "dtout": dt}


# ---- scene flow -----------------------------------------------------------------------------------------------------------------------
def sf_case(lay, kind, n, seed=0, box=BOX_POW2, enc="normal", gf=True, gb=True, prefill=True):
    """as warp_case: 'exact' (integers; g_pts pre-filled with integers in [0, 4] unless prefill is False), 'dense', 'gate_edges' (rows
    H0 / H2 / H4 from GATES)"""
    T = (n + 31) // 32
    rng = np.random.default_rng([47, ("exact", "dense", "gate_edges").index(kind), seed, n])
    if kind == "exact":
        rows = rng.integers(-2, 3, size=(T, lay["rows"], 32)).astype(f32)
        W = list(_int_weights(rng, dict(enumerate(SF_SHAPES))).values())
        g_f, g_b = rng.integers(-1, 2, size=(n, 3)).astype(f32), rng.integers(-1, 2, size=(n, 3)).astype(f32)
        pre = rng.integers(0, 5, size=(n, 3)).astype(f32)
    else:
        rows = rng.standard_normal((T, lay["rows"], 32), dtype=f32)
        W = [(rng.standard_normal(s, dtype=f32) / f32(np.sqrt(s[1]))).astype(f32) for s in SF_SHAPES]
        g_f, g_b = rng.standard_normal((n, 3), dtype=f32), rng.standard_normal((n, 3), dtype=f32)
        pre = rng.integers(-3, 4, size=(n, 3)).astype(f32)
        if enc == "sincos":
            xn = rng.uniform(-1.0, 1.0, size=(n, 3)).astype(f32)
            q = np.stack([np.ldexp(xn[:, d], f) for d in range(3) for f in range(4)], -1).astype(f32).astype(f64)
            put_rows(rows, lay["X"][:27], np.concatenate([xn, np.sin(q).astype(f32), np.cos(q).astype(f32)], -1))
        if kind == "gate_edges":
            for key in ("H0", "H2", "H4"):
                put_rows(rows, lay[key], GATES[rng.integers(0, len(GATES), size=(n, 64))])
    if not prefill:
        pre = np.zeros((n, 3), dtype=f32)
    c = dict(kind=kind, n=n, rows=rows, W=W, gf=g_f if gf else None, gb=g_b if gb else None, pre=pre, box=np.asarray(box, dtype=f32))
    if kind == "exact":
        c["max_quanta"] = sf_exact_guard(c, lay)
    return c


def sf_exact_guard(c, lay):
    """as warp_exact_guard: everything up to e is an integer; g_pts is a multiple of 2^-2 on a box whose inv are powers of two, and
    on any other box with a zero pre-fill it is the single product fl32(e inv), e exact"""
    r = sf_reference(c, lay)
    inv = box_inv(c["box"]).astype(f64)
    pow2 = all(v in (0.25, 0.5, 1.0) for v in inv)
    assert pow2 or not np.any(c["pre"])
    worst = max([float(r["cond"][k].max(initial=0.0)) for k in ("dz4", "dz2", "dz0", "dX", "e")] +
                [float(r["cond"]["g_pts"].max(initial=0.0)) * 4 if pow2 else 0.0])
    assert worst < 2 ** 24, worst
    return worst


def _sf_inputs(c, lay, dtype):
    n = c["n"]
    a = samples(c["rows"], n).astype(dtype)
    dz6 = np.zeros((n, 6), dtype=dtype)
    if c["gf"] is not None:
        dz6[:, :3] = c["gf"]
    if c["gb"] is not None:
        dz6[:, 3:] = c["gb"]
    W = [w.astype(dtype) for w in c["W"]]
    pre = np.zeros((n, 3), dtype=dtype) if c.get("pre") is None else c["pre"].astype(dtype)
    return n, a[:, lay["X"]], a[:, lay["H0"]] > 0, a[:, lay["H2"]] > 0, a[:, lay["H4"]] > 0, W, dz6, pre


SF_TIME_COLS = [(28 + f, 32 + f) for f in range(4)]   # [.. | t 27 | sin(2^f t) | cos]: the model's definition of the input


def sf_reference(c, lay):
    """-> {'g_pts': (value [n][3], bound), 'e': (value, bound): the gradient of the normalised point, 'cond': {...}}"""
    n, X, G0, G2, G4, W, dz6, pre = _sf_inputs(c, lay, f64)
    inv = box_inv(c["box"]).astype(f64)[None, :]
    A = [np.abs(w) for w in W]
    cond = {}
    dz4 = np.where(G4, dz6 @ W[3], 0.0)
    cond["dz4"] = np.where(G4, np.abs(dz6) @ A[3], 0.0)
    b4 = 6 * U * cond["dz4"]
    dz2 = np.where(G2, dz4 @ W[2], 0.0)
    cond["dz2"] = np.where(G2, np.abs(dz4) @ A[2], 0.0)
    b2 = np.where(G2, b4 @ A[2] + 64 * U * cond["dz2"], 0.0)
    dz0 = np.where(G0, dz2 @ W[1], 0.0)
    cond["dz0"] = np.where(G0, np.abs(dz2) @ A[1], 0.0)
    b0 = np.where(G0, b2 @ A[1] + 64 * U * cond["dz0"], 0.0)
    dX = dz0 @ W[0]
    cond["dX"] = np.abs(dz0) @ A[0]
    bX = b0 @ A[0] + 64 * U * cond["dX"]
    e, cond["e"], be = pe_backward(X, dX, bX, 4, 4)
    g = pre + e * inv
    cond["g_pts"] = np.abs(pre) + cond["e"] * inv
    bg = be * inv + 2 * U * cond["g_pts"]
    return {"g_pts": (g, _finish(bg, cond["g_pts"])), "e": (e, _finish(be, cond["e"])), "cond": cond,
            "dX": (dX, _finish(bX, cond["dX"]))}


def sf_eval32(c, lay, mut=()):
    """-> {'g_pts' [n][3]} in float32; mut: wrong kernels (MUTATIONS)"""
    n, X, G0, G2, G4, W, dz6, pre = _sf_inputs(c, lay, f32)
    inv = _mut_inv(box_inv(c["box"]), mut)[None, :]
    zero = f32(0.0)
    dz4 = np.where(G4, MP.seq32(dz6, np.ascontiguousarray(W[3].T)), zero)
    dz2 = np.where(G2, MP.seq32(dz4, np.ascontiguousarray(W[2].T)), zero)
    dz0 = np.where(G0, MP.seq32(dz2, np.ascontiguousarray(W[1].T)), zero)
    dX = MP.seq32(dz0, np.ascontiguousarray(W[0].T))
    e = pe_backward32(X, dX, 4, mut, SF_TIME_COLS)
    g = (pre + (e * (np.ones_like(inv) if "no_inv_g" in mut else inv)).astype(f32)).astype(f32)
    assert g.dtype == f32
    return {"g_pts": g, "e": e}
