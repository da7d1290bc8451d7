"""Float64 references, seeded generators and derived bounds for two links of the dynamic field's density-phase backward, shared by
test_heads_primitives_cpu.py and test_gpu_heads_primitives.py.  No GPU.
  * the heads' backward tile (dyn_heads_bwd_tile behind rdrf_selftest_heads_bwd: k_dyn_density_bwd<0, false, true> on flat tiles,
    k_dyn_density_bwd<0, true> in feature mode);
  * the time branch, forward (time_branch_body behind rdrf_selftest_time_branch) and backward (k_time_branch_bwd with
    dtout_of_ray behind rdrf_selftest_time_branch_bwd).
Every reference takes the float32 inputs the kernel gets, widens them to float64 and returns, per output, the value and an absolute
bound  k 2^-24 cond (+ what its inputs' own bounds contribute), cond being the sum of the absolute values of the terms added and k
the count of the kernel's rounded operations on the way, written out where it is formed.  U = 2^-24 is the unit roundoff of one
fp32 operation.  An output whose cond is 0 has the bound 0: it must be exactly 0.  Where a term can fall below the smallest normal
number (a product with 2^-126) TINY = 2^-126 per term is added: such a term may be flushed.  No constant was tuned against the kernels.

Layouts are never written down here: the rows of a tile come from rdrf_selftest_dw_describe (dz rows, saved activation rows, the
first layer's column of every d(feature) / d(X0) row), rdrf_selftest_scatter_describe (the d(feature) rows, their level / plane /
component and their offset in a sample-major record) and rdrf_selftest_heads_describe (d(X0) rows, small-layer dz rows, launch
geometry).

Heads.  g_fd = valid ? gsig act'(fd) : 0, act' = [fd > 0] (relu: exact, k = 1 for the product) or sigmoid(fd + shift) (softplus: x =
fd + shift rounds once, which moves the sigmoid by at most |x| U of itself; expf within 2 ulp = 4 U, 1 + e and the division one
each: k = |x| + 6, and 1 for the product).  g_fb = valid ? g_b bl (1 - bl) : 0: bl carries (|fb| + 6) U, and 1 - bl is a SUM of the
terms 1 and bl, so cond = |g_b| bl (1 + bl) and k = |fb| + 6 + 3 (the difference and two products).  Feature mode hands both in: exact.
dz[k] = H[k] > 0 ? w2[k] g : 0: the bound of g times |w2[k]|, and U |dz| for the product.  dF and dX0 are the backward-data products
of the first layer, the mfma_seg_b3_pair<3, 2, 32> form that tests/_mlp_prim.py bounds as B3_PAIR_T (160, 64): b3_pair_bound imports
its two bounds -- 2 e_seq32 of the same inputs for the accumulation, ONE_HOT_BOUND for the dropped piece products -- and adds
them; dX0 adds the two heads in one accumulator (U cond more).  The small layers: dw2[k] += sum g H[k] is a product (1), the five
butterfly stages of reduce_scatter32 (5), the wave's running sum over its tiles (tiles per wave), the LDS sum over the workgroup's
waves (waves) and one atomic per workgroup onto the pre-fill (workgroups); db2 += sum g is the running sum (tiles per wave), the six
stages of wave_sum (6), waves and workgroups.  Geometry: rdrf_selftest_heads_describe.

Time branch.  tin = [t, sin(2^f t), cos(2^f t)]: ldexp is exact, sincosf gets the allowance tests/_gather_prim.py gives the encodings'
OCML path (PE_OCML_BOUND, absolute).  pre = b1 + W1 tin is a chain of 17 fma (k = 17), h = relu(pre) keeps pre's bound, tout = b2 + W2 h
a chain of 64 (k = 64); columns 30 and 31 of tout are stored as 0.  Backward: d(tout) of a ray is dtout[n], or the sum of its tiles'
partial records in tile order (one rounding per record after the first); dh = W2^T dz2 is a chain of 30; the four parameter
gradients sum 32 rays per workgroup in a chain (32) and add one atomic per workgroup onto the pre-fill (workgroups).  The relu gate
of the backward is recomputed in fp32, so the generator only builds inputs whose every (ray, neuron) pre is exactly 0 by
construction (a zero weight row with a zero bias) or at least GATE_MARGIN = 16 forward bounds of pre away from 0 (deterministic
re-draws of t): no case is excluded at comparison time, and test_heads_primitives_cpu.py asserts the margin."""
import ctypes as C

import numpy as np

import _dw_prim as DW
import _gather_prim as GP
import _mlp_prim as MP
import _scatter_prim as SC

f32, f64 = np.float32, np.float64
U = 2.0 ** -24
TINY = 2.0 ** -126
SINCOS = GP.PE_OCML_BOUND
GATE_MARGIN = 16.0
SHIFT = -10.0
NAN = np.frombuffer(b"\xff\xff\xff\xff", dtype=f32)[0]   # the pre-fill of every output: a NaN pattern

FLAT_SHAPES = [(1, 1), (1, 32), (3, 11), (5, 13), (35, 33)]
FLAT_WAVES = (257, 33)     # 266 tiles: two waves per workgroup, so the LDS sum over a workgroup's waves has two terms
FLAT_WALK = (1987, 33)     # 2050 tiles on 256 x 8 waves: some waves walk a second tile (running sums, the persistent stride)
FEAT_SIZES = [1, 31, 32, 33, 70]
LIVE_SETS = [("d",), ("b",), ("d", "b")]
TB_FWD_N = [1, 7, 8, 9, 35]
TB_FIXED_T = [0.0, 1.0, -1.0, 1.0 - 2.0 ** -24, 0.5, -0.37]
TB_BWD_N = [1, 31, 32, 33, 65]
TB_BWD_S = [1, 5, 31, 32, 33, 70]
RELU_FD = [0.0, 2.0 ** -126, -2.0 ** -126, 1.0, -1.0]
LOGITS = [-90.0, -20.0, 0.0, 20.0, 90.0]


# ---- layouts from the library --------------------------------------------------------------------------------------------------
def heads_describe(L, mode, N, S=1):
    buf = (C.c_int * 16)()
    n = L.lib.rdrf_selftest_heads_describe(int(mode), int(N), int(S), buf, 16)
    if n < 0:
        raise RuntimeError(f"rdrf_selftest_heads_describe: rc {n}: {L.lib.rdrf_last_error().decode()}")
    assert buf[0] == n
    return dict(zip(("grid", "waves", "tiles", "rows", "grows", "dx0", "sm", "rec"), buf[1:n]))


def layout(L):
    """row offsets of a tile, per head (0 density, 1 blending): H[head][k] saved row of hidden unit k, DZ[head] first dz row,
    SM[head] the small-layer dz row, DF[head] first d(feature) row, fcols [96] / xcols [64]: first-layer column of each d(feature) /
    d(X0) row (-1: padding), fmap: per feature (row, level, plane, component, record slot), set_floats: a head's part of a record"""
    d = DW.describe(L, "DENSITY", L.DW_LIVE_D | L.DW_LIVE_B)
    sd = SC.describe(L, "DYN_DENSITY")
    hd = heads_describe(L, 0, 1, 1)
    nfeat = sd["nfeat"]
    off = {n: getattr(L.RdrfDynamicParams, n).offset for n in ("dw1", "bw1", "dw2", "bw2")}

    def job(name):
        js = [j for j in d["jobs"] if j["w_off"] == off[name]]
        assert len(js) == 1, name
        return js[0]

    lay = dict(rows=hd["rows"], grows=hd["grows"], DX0=hd["dx0"], rec=hd["rec"], set_floats=sd["set_floats"], nfeat=nfeat,
               H=[], DZ=[], SM=[], DF=list(sd["row0"]), fmap=SC.feature_map(sd))
    for head, (big, small) in enumerate((("dw1", "dw2"), ("bw1", "bw2"))):
        js, jb = job(small), job(big)
        assert js["out_dim"] == 1 and js["A_row0"] == hd["sm"] and jb["out_dim"] == 64 and jb["in_dim"] == 152
        Hrow = np.full(64, -1, dtype=np.int64)
        for row0, cols in js["blocks"]:
            Hrow[np.asarray(cols)] = row0 + np.arange(32)
        assert (Hrow >= 0).all()
        lay["H"].append(Hrow)
        lay["DZ"].append(jb["A_row0"])
        lay["SM"].append(js["A_row0"] + js["out_row0"])
        fb = [(r, np.asarray(c)) for r, c in jb["blocks"] if c.max() < nfeat]
        xb = [(r, np.asarray(c)) for r, c in jb["blocks"] if nfeat <= c.max() < nfeat + 64]
        fcols, xcols = np.concatenate([c for _, c in fb]), np.concatenate([c for _, c in xb])
        assert [r - fb[0][0] for r, _ in fb] == [0, 32, 64] and [r - xb[0][0] for r, _ in xb] == [0, 32]
        assert sorted(fcols[fcols >= 0]) == list(range(nfeat)) and sorted(xcols[xcols >= 0]) == list(range(nfeat, nfeat + 64))
        if head == 0:
            lay["fcols"], lay["xcols"] = fcols, xcols
        else:   # both heads read the same saved rows in the same order
            assert np.array_equal(fcols, lay["fcols"]) and np.array_equal(xcols, lay["xcols"])
    return lay


def rows_of(arr, row0, count, n):
    """[T][R][32] rows -> [n][count]: sample i = 32 tile + lane"""
    T = arr.shape[0]
    return arr[:, row0:row0 + count, :].transpose(0, 2, 1).reshape(T * 32, count)[:n]


# ---- heads: inputs ---------------------------------------------------------------------------------------------------------------
def heads_weights(seed=0):
    rng = np.random.default_rng([23, seed])
    return {"dw1": (rng.standard_normal((64, 152), dtype=f32) / f32(np.sqrt(152.0))).astype(f32),
            "bw1": (rng.standard_normal((64, 152), dtype=f32) / f32(np.sqrt(152.0))).astype(f32),
            "dw2": (rng.standard_normal((1, 64), dtype=f32) / f32(8.0)).astype(f32),
            "bw2": (rng.standard_normal((1, 64), dtype=f32) / f32(8.0)).astype(f32)}


def heads_case(mode, N, S, act, live, seed=0, regime="edges"):
    """mode 'flat': N rays of S samples; 'feat': N points.  live: subset of ('d', 'b').  regime 'edges': gate values {+0, -0, 2^-126,
    ordinary of both signs} next to each other in the saved H rows (denormals are left out: whether the hardware flushes a denormal
    input of the comparison is not part of the contract), the activation's edge values in every third sample, invalid samples; 'int':
    small integers with act' = 1 and bl (1 - bl) = 1/4 exactly, for the exact sums of the small layers (relu only)."""
    n = N * S if mode == "flat" else N
    rng = np.random.default_rng([29, seed, N, S, len(live), int(act == "relu")])
    c = dict(mode=mode, N=N, S=S if mode == "flat" else 1, n=n, act=act, shift=SHIFT, live_d="d" in live, live_b="b" in live, regime=regime)
    if regime == "int":
        assert act == "relu"
        H = rng.integers(-2, 3, size=(2, n, 64)).astype(f32)
        raw = np.tile(np.array([1.0, 0.0], dtype=f32), (n, 1))
        gs, gb = rng.integers(-3, 4, size=n).astype(f32), (4 * rng.integers(-3, 4, size=n)).astype(f32)
        valid = (rng.random(n) < 0.85).astype(np.uint8)
    else:
        kind = rng.choice(5, size=(2, n, 64), p=[0.15, 0.15, 0.15, 0.35, 0.2])
        mag = np.abs(rng.standard_normal((2, n, 64), dtype=f32)) + f32(2.0 ** -20)
        H = np.select([kind == 0, kind == 1, kind == 2, kind == 3], [f32(0.0), f32(-0.0), f32(TINY), mag], -mag).astype(f32)
        raw = (3.0 * rng.standard_normal((n, 2))).astype(f32)
        if act == "softplus":
            raw[:, 0] -= f32(SHIFT)   # fd + shift of order 3: both tails of the sigmoid
        i3 = np.arange(0, n, 3)
        fd_edges = np.array(RELU_FD if act == "relu" else [v - SHIFT for v in LOGITS], dtype=f32)
        raw[i3, 0] = fd_edges[(i3 // 3 + seed) % 5]
        raw[i3, 1] = np.array(LOGITS, dtype=f32)[(i3 // 3 + seed + i3 // 15) % 5]
        gs, gb = rng.standard_normal(n, dtype=f32), rng.standard_normal(n, dtype=f32)
        valid = (rng.random(n) < 0.8).astype(np.uint8)
        valid[i3] = 1
        if n > 1:
            valid[1] = 0
        valid[n - 1] = 1   # (3, 11): the one live lane of the second tile
    c.update(H=H, raw=raw, valid=valid)
    if mode == "flat":
        c["gsig"], c["g_b"] = gs, (gb if c["live_b"] else None)
    else:
        c["g_sigma"], c["g_b"] = (gs if c["live_d"] else None), (gb if c["live_b"] else None)
    return c


def heads_rows(c, lay, pad=3e38):
    """the saved rows [T][rows][32] the kernel is handed: NaN in every row it must not read, `pad` in the lanes past n"""
    n, T = c["n"], (c["n"] + 31) // 32
    act = np.full((T, lay["rows"], 32), NAN, dtype=f32)
    for head in range(2):
        full = np.full((T * 32, 64), f32(pad), dtype=f32)
        full[:n] = c["H"][head]
        act[:, lay["H"][head], :] = full.reshape(T, 32, 64).transpose(0, 2, 1)
    return act


# ---- heads: reference --------------------------------------------------------------------------------------------------------------
def _sigmoid(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def b3_pair_bound(x32, We):
    """the relative bound (of sum |x| |w|) of the mfma_seg_b3_pair<3, 2, 32> products: the two bounds tests/_mlp_prim.py holds
    B3_PAIR_T (160, 64) to, added -- 2 e_seq32 (dense rows: the accumulation) and ONE_HOT_BOUND (the piece products the scheme drops)"""
    return 2.0 * MP.e_seq32(np.ascontiguousarray(x32, dtype=f32), np.ascontiguousarray(We, dtype=f32)) + MP.ONE_HOT_BOUND


def head_out_grads(c):
    """-> (g [2][n], bound [2][n]) of the raw outputs"""
    n = c["n"]
    raw, valid = np.asarray(c["raw"], dtype=f64), np.asarray(c["valid"]) != 0
    g, b = np.zeros((2, n)), np.zeros((2, n))
    if c["mode"] == "feat":   # handed in: exact
        for head, key in enumerate(("g_sigma", "g_b")):
            if c[key] is not None:
                g[head] = np.asarray(c[key], dtype=f64)
        return g, b
    gs = np.asarray(c["gsig"], dtype=f64)
    if c["act"] == "relu":
        g[0] = np.where(valid & (raw[:, 0] > 0), gs, 0.0)
        b[0] = 1 * U * np.abs(g[0])
    else:
        x = raw[:, 0] + c["shift"]
        g[0] = np.where(valid, gs * _sigmoid(x), 0.0)
        b[0] = (np.abs(x) + 6 + 1) * U * np.abs(g[0]) + TINY * (g[0] != 0)
    if c["g_b"] is not None:
        gb, bl = np.asarray(c["g_b"], dtype=f64), _sigmoid(raw[:, 1])
        g[1] = np.where(valid, gb * bl * (1.0 - bl), 0.0)
        b[1] = np.where(valid, (np.abs(raw[:, 1]) + 6 + 3) * U * np.abs(gb) * bl * (1.0 + bl), 0.0) + TINY * (g[1] != 0)
    return g, b


def heads_reference(c, lay, W, geo=None, pre=None):
    """-> {name: (value, bound)}: 'sm' [n][2], 'dz' / 'dF' [2][n][64 / 96] in row order (meaningful for the live heads), 'dX0' [n][64],
    and with geo (heads_describe of the launch) and pre (the pre-fill) 'dw2', 'bw2' [64], 'db2', 'bb2' [1]"""
    n = c["n"]
    g, bg = head_out_grads(c)
    live = (c["live_d"], c["live_b"])
    out = {"sm": (g.T.copy(), bg.T.copy())}
    dz, bdz, dF, bdF = np.zeros((2, n, 64)), np.zeros((2, n, 64)), np.zeros((2, n, 96)), np.zeros((2, n, 96))
    dX, bdX, condX = np.zeros((n, 64)), np.zeros((n, 64)), np.zeros((n, 64))
    cols = np.concatenate([lay["fcols"], lay["xcols"]])
    for head in range(2):
        if not live[head]:
            continue
        H = np.asarray(c["H"][head], dtype=f64)
        w1 = np.asarray(W["dw1" if head == 0 else "bw1"], dtype=f64)
        w2 = np.asarray(W["dw2" if head == 0 else "bw2"], dtype=f64).reshape(64)
        gate = H > 0
        dz[head] = np.where(gate, w2[None, :] * g[head][:, None], 0.0)
        bdz[head] = np.where(gate, np.abs(w2)[None, :] * bg[head][:, None] + U * np.abs(dz[head]) + TINY * (dz[head] != 0), 0.0)
        We = np.where(cols[:, None] >= 0, w1[:, np.maximum(cols, 0)].T, 0.0)   # [160][64]: the transposed form's effective weight
        y, cond = dz[head] @ We.T, np.abs(dz[head]) @ np.abs(We).T
        rel = b3_pair_bound(dz[head].astype(f32), We.astype(f32))
        by = bdz[head] @ np.abs(We).T + rel * cond + TINY * (cond > 0)
        dF[head], bdF[head] = y[:, :96], by[:, :96]
        dX += y[:, 96:]
        bdX += by[:, 96:]
        condX += cond[:, 96:]
    if live[0] and live[1]:
        bdX += U * condX   # the second head's products land on the first head's sums
    out.update(dz=(dz, bdz), dF=(dF, bdF), dX0=(dX, bdX))
    if geo is not None and c["mode"] == "flat":
        tpw = -(-geo["tiles"] // (geo["grid"] * geo["waves"]))
        kw, kb = 1 + 5 + tpw + geo["waves"] + geo["grid"], tpw + 6 + geo["waves"] + geo["grid"]
        for head, (wn, bn) in enumerate((("dw2", "db2"), ("bw2", "bb2"))):
            pw, pb = np.asarray(pre[wn], dtype=f64).reshape(64), np.asarray(pre[bn], dtype=f64).reshape(1)
            if not live[head]:
                out[wn], out[bn] = (pw, np.zeros(64)), (pb, np.zeros(1))
                continue
            H = np.asarray(c["H"][head], dtype=f64)
            terms = g[head][:, None] * H
            cw, cb = np.abs(pw) + np.abs(terms).sum(0), np.abs(pb) + np.abs(g[head]).sum()
            out[wn] = (pw + terms.sum(0), (bg[head][:, None] * np.abs(H)).sum(0) + kw * U * cw + TINY * (terms != 0).sum(0))
            out[bn] = (pb + g[head].sum(), bg[head].sum() + kb * U * cb)
    return out


def _tree32(v):
    """float32 sum over the last axis (a power of two long) in butterfly stages: log2 additions on every path"""
    v = np.asarray(v, dtype=f32)
    while v.shape[-1] > 1:
        v = (v[..., 0::2] + v[..., 1::2]).astype(f32)
    return v[..., 0]


def small_sums32(g, H, geo, pw, pb):
    """dw2 / db2 of one head in float32 in the kernel's order: per tile the products and a butterfly over the 32 lanes; a wave's
    running sum over the tiles it walks (wg * waves + wave, + grid * waves, ...); the sum over the workgroup's waves; one addition
    per workgroup onto the pre-fill.  g [n], H [n][64] float32; geo: heads_describe of the launch"""
    T, grid, waves = geo["tiles"], geo["grid"], geo["waves"]
    gt, Ht = np.zeros((T * 32,), dtype=f32), np.zeros((T * 32, 64), dtype=f32)
    gt[:len(g)], Ht[:len(g)] = g, H
    gt, Ht = gt.reshape(T, 32), Ht.reshape(T, 32, 64)
    tw = _tree32((gt[:, :, None] * Ht).astype(f32).transpose(0, 2, 1))   # [T][64]
    accw, accb = np.asarray(pw, dtype=f32).reshape(64).copy(), np.asarray(pb, dtype=f32).reshape(1).copy()
    for wg in range(grid):
        vw, vb = np.zeros(64, dtype=f32), f32(0.0)
        for wave in range(waves):
            sw, sb = np.zeros(64, dtype=f32), np.zeros(32, dtype=f32)
            for tl in range(wg * waves + wave, T, grid * waves):
                sw, sb = sw + tw[tl], sb + gt[tl]
            vw, vb = vw + sw, f32(vb + _tree32(sb))
        accw, accb = accw + vw, accb + vb
    assert accw.dtype == f32 and accb.dtype == f32
    return accw, accb


def heads_eval32(c, lay, W, geo=None, pre=None):
    """the same operation evaluated in plain float32 (numpy; the products sequentially, the small-layer sums in the kernel's order):
    what test_heads_primitives_cpu.py holds to the bounds"""
    n = c["n"]
    raw, valid = c["raw"].astype(f32), c["valid"] != 0
    g = np.zeros((2, n), dtype=f32)
    one = f32(1.0)
    if c["mode"] == "feat":
        for head, key in enumerate(("g_sigma", "g_b")):
            if c[key] is not None:
                g[head] = c[key]
    else:
        with np.errstate(over="ignore"):
            if c["act"] == "relu":
                ad = (raw[:, 0] > 0).astype(f32)
            else:
                ad = one / (one + np.exp(-(raw[:, 0] + f32(c["shift"])), dtype=f32))
            g[0] = np.where(valid, c["gsig"] * ad, f32(0.0))
            if c["g_b"] is not None:
                bl = one / (one + np.exp(-raw[:, 1], dtype=f32))
                g[1] = np.where(valid, c["g_b"] * bl * (one - bl), f32(0.0))
    out = {"sm": g.T.copy()}
    cols = np.concatenate([lay["fcols"], lay["xcols"]])
    dz, dF, dX = np.zeros((2, n, 64), dtype=f32), np.zeros((2, n, 96), dtype=f32), np.zeros((n, 64), dtype=f32)
    for head, (live, names) in enumerate(zip((c["live_d"], c["live_b"]), (("dw1", "dw2", "db2"), ("bw1", "bw2", "bb2")))):
        if not live:
            continue
        w1, w2 = W[names[0]], W[names[1]].reshape(64)
        dz[head] = np.where(c["H"][head] > 0, w2[None, :] * g[head][:, None], f32(0.0))
        We = np.where(cols[:, None] >= 0, w1[:, np.maximum(cols, 0)].T, f32(0.0)).astype(f32)
        y = MP.seq32(dz[head], We)
        dF[head] = y[:, :96]
        dX = dX + y[:, 96:]
        if geo is not None and c["mode"] == "flat":
            out[names[1]], out[names[2]] = small_sums32(g[head], c["H"][head], geo, pre[names[1]], pre[names[2]])
    out.update(dz=dz, dF=dF, dX0=dX)
    return out


def ratio(got, ref, bound):
    """max |got - ref| / bound over the elements; an element whose bound is 0 must be met exactly (then 0, else inf)"""
    got, ref, bound = np.asarray(got, dtype=f64), np.asarray(ref, dtype=f64), np.asarray(bound, dtype=f64)
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    if got.size == 0:
        return 0.0
    if not np.isfinite(got).all():
        return float("inf")
    err = np.abs(got - ref)
    if (err[bound == 0] != 0).any():
        return float("inf")
    return float((err / np.where(bound == 0, 1.0, bound)).max())


# ---- time branch ---------------------------------------------------------------------------------------------------------------------
def tb_weights(seed=0, zero_rows=()):
    """time_layer1 [64][17] + [64], time_layer2 [30][64] + [30]; zero_rows: hidden neurons with a zero weight row and a zero bias"""
    rng = np.random.default_rng([31, seed])
    W = {"l1w": (rng.standard_normal((64, 17), dtype=f32) / f32(np.sqrt(17.0))).astype(f32), "l1b": (0.3 * rng.standard_normal(64, dtype=f32)).astype(f32),
         "l2w": (rng.standard_normal((30, 64), dtype=f32) / f32(8.0)).astype(f32), "l2b": (0.3 * rng.standard_normal(30, dtype=f32)).astype(f32)}
    for k in zero_rows:
        W["l1w"][k] = 0.0
        W["l1b"][k] = 0.0
    return W


def tb_tin(t):
    """-> tin [N][17] float64 from the float32 t, and the absolute bound of each entry"""
    t = np.asarray(t, dtype=f32).reshape(-1)
    q = np.stack([np.ldexp(t, f) for f in range(8)], -1).astype(f32).astype(f64)   # exact in float32
    tin = np.concatenate([t.astype(f64)[:, None], np.sin(q), np.cos(q)], -1)
    btin = np.concatenate([np.zeros((t.size, 1)), np.full((t.size, 16), SINCOS)], -1)
    return tin, btin


def tb_forward(W, t):
    """-> dict: tin, btin, pre, bpre [N][64], h, tout [N][32] (columns 30, 31 zero), btout"""
    w1, b1, w2, b2 = (np.asarray(W[k], dtype=f64) for k in ("l1w", "l1b", "l2w", "l2b"))
    tin, btin = tb_tin(t)
    pre = tin @ w1.T + b1
    bpre = btin @ np.abs(w1).T + 17 * U * (np.abs(tin) @ np.abs(w1).T + np.abs(b1))
    h = np.maximum(pre, 0.0)
    tout, btout = np.zeros((tin.shape[0], 32)), np.zeros((tin.shape[0], 32))
    tout[:, :30] = h @ w2.T + b2
    btout[:, :30] = bpre @ np.abs(w2).T + 64 * U * (h @ np.abs(w2).T + np.abs(b2))
    return dict(tin=tin, btin=btin, pre=pre, bpre=bpre, h=h, tout=tout, btout=btout)


def ray_tiles(N, S):
    """per ray: (first tile, last tile, slot of its record in the first tile: 0 if the ray starts the tile, else 1)"""
    b = np.arange(N) * S
    return b >> 5, (b + S - 1) >> 5, np.where((b & 31) == 0, 0, 1)


def dtout_of_ray(dtout, dtp, N, S):
    """reference of dtout_of_ray (csrc/rdrf_bwd.hip): -> d(tout) [N][30] float64 and cond, the sum of the absolute records, and the
    number of records summed per ray"""
    dtout = np.asarray(dtout, dtype=f64)
    if dtp is None:
        return dtout[:, :30].copy(), np.abs(dtout[:, :30]), np.ones(N, dtype=np.int64)
    dtp = np.asarray(dtp, dtype=f64)
    t0, t1, slot = ray_tiles(N, S)
    v, cond, cnt = np.zeros((N, 30)), np.zeros((N, 30)), np.ones(N, dtype=np.int64)
    for n in range(N):
        if t0[n] == t1[n]:
            v[n], cond[n] = dtout[n, :30], np.abs(dtout[n, :30])
            continue
        recs = [dtp[t0[n], slot[n], :30]] + [dtp[t, 0, :30] for t in range(t0[n] + 1, t1[n] + 1)]   # in tile order
        v[n], cond[n], cnt[n] = np.sum(recs, 0), np.abs(recs).sum(0), len(recs)
    return v, cond, cnt


def tb_backward(W, t, S, dtout, dtp, pre_fill):
    """-> {name: (value, bound)} of the four gradients, added into pre_fill; plus 'fwd' (tb_forward) and 'gate' [N][64]"""
    w1, w2 = np.asarray(W["l1w"], dtype=f64), np.asarray(W["l2w"], dtype=f64)
    N = np.asarray(t).size
    fw = tb_forward(W, t)
    dz2, c2, cnt = dtout_of_ray(dtout, dtp, N, S)
    bdz2 = (cnt - 1)[:, None] * U * c2
    gate = fw["pre"] > 0
    dh = dz2 @ w2
    bdh = bdz2 @ np.abs(w2) + 30 * U * (np.abs(dz2) @ np.abs(w2))
    dz1, bdz1 = np.where(gate, dh, 0.0), np.where(gate, bdh, 0.0)
    k = 32 + (N + 31) // 32
    h, bh, tin, btin = fw["h"], np.where(gate, fw["bpre"], 0.0), fw["tin"], fw["btin"]

    def prod(a, ba, b, bb, key):
        p = np.asarray(pre_fill[key], dtype=f64)
        val = p + (a.T @ b).reshape(p.shape)
        cond = np.abs(p) + (np.abs(a).T @ np.abs(b)).reshape(p.shape)
        inp = ((np.abs(a) + ba).T @ (np.abs(b) + bb) - np.abs(a).T @ np.abs(b)).reshape(p.shape)
        return val, inp + k * U * cond

    ones, zeros = np.ones((N, 1)), np.zeros((N, 1))
    return {"l2w": prod(dz2, bdz2, h, bh, "l2w"), "l1w": prod(dz1, bdz1, tin, btin, "l1w"), "l2b": prod(dz2, bdz2, ones, zeros, "l2b"),
            "l1b": prod(dz1, bdz1, ones, zeros, "l1b"), "fwd": fw, "gate": gate}


def gate_margin(W, t):
    """min over the (ray, neuron) pairs whose pre is not exactly 0 by construction of |pre| / bound(pre); inf if there is none"""
    fw = tb_forward(W, t)
    zero_row = (np.asarray(W["l1w"]) == 0).all(-1) & (np.asarray(W["l1b"]) == 0)
    m = np.abs(fw["pre"])[:, ~zero_row] / fw["bpre"][:, ~zero_row]
    assert (fw["pre"][:, zero_row] == 0).all()
    return float(m.min()) if m.size else float("inf")


def tb_times(W, N, seed=0, margin=GATE_MARGIN):
    """N seeded times in [-1, 1] whose every pre is exactly 0 by construction or at least `margin` bounds away from 0: a time that
    fails is drawn again from the same stream (deterministic); -> t [N] float32, the number of re-draws"""
    rng = np.random.default_rng([37, seed, N])
    t, redraws = np.empty(N, dtype=f32), 0
    for n in range(N):
        while True:
            t[n] = f32(rng.uniform(-1.0, 1.0))
            if gate_margin(W, t[n:n + 1]) >= margin:
                break
            redraws += 1
            assert redraws < 64 * N, "the gate classes cannot be met"
    return t, redraws


def tb_cotangents(N, S, with_dtp, seed=0):
    """dtout [N][32] and dtp [T][2][32] (or None) holding a seeded value in exactly the slots dtout_of_ray reads and NaN in every other
    one: the rays inside one tile in dtp, the crossing rays in dtout, the unused record of each tile, columns 30 and 31"""
    rng = np.random.default_rng([41, seed, N, S])
    T = (N * S + 31) // 32
    dtout = np.full((N, 32), NAN, dtype=f32)
    dtp = np.full((T, 2, 32), NAN, dtype=f32) if with_dtp else None
    t0, t1, slot = ray_tiles(N, S)
    for n in range(N):
        if not with_dtp or t0[n] == t1[n]:
            dtout[n, :30] = rng.standard_normal(30, dtype=f32)
        else:
            dtp[t0[n], slot[n], :30] = rng.standard_normal(30, dtype=f32)
            for tl in range(t0[n] + 1, t1[n] + 1):
                dtp[tl, 0, :30] = rng.standard_normal(30, dtype=f32)
    return dtout, dtp


def tile_records(per_sample, N, S):
    """what the flat warp tile writes (k_dyn_density_bwd<1, false, true>): per_sample [N S][30] -> dtout [N][32], dtp [T][2][32] with
    NaN where nothing is written.  Brute force, sample by sample: a tile's samples are grouped by ray; a ray inside the tile goes to
    dtout, the others to the tile's record 0 (the group starts the tile) or 1."""
    T = (N * S + 31) // 32
    dtout, dtp = np.full((N, 32), np.nan), np.full((T, 2, 32), np.nan)
    for tl in range(T):
        i = 32 * tl
        while i < min(32 * tl + 32, N * S):
            ray, j = i // S, i
            acc = np.zeros(30)
            while j < min(32 * tl + 32, N * S) and j // S == ray:
                acc += per_sample[j]
                j += 1
            inside = ray * S >= 32 * tl and ray * S + S - 1 <= 32 * tl + 31
            if inside:
                dtout[ray, :30] = acc
            else:
                dtp[tl, 0 if i == 32 * tl else 1, :30] = acc
            i = j
    return dtout, dtp


def fma32(a, b, c):
    """fmaf on float32 arrays: the product is exact in float64, the sum rounds there once more before it rounds to float32"""
    return (np.asarray(a, dtype=f64) * np.asarray(b, dtype=f64) + np.asarray(c, dtype=f64)).astype(f32)


def tb_eval32(W, t, S=None, dtout=None, dtp=None, pre_fill=None):
    """the time branch in float32 in the kernels' order (numpy sin / cos, fma chains of 17, 64, 30; 32 rays per workgroup summed in a
    chain, one addition per workgroup onto the pre-fill): -> pre, tout [N][30], and with cotangents the four gradients"""
    t = np.asarray(t, dtype=f32).reshape(-1)
    N = t.size
    q = np.stack([np.ldexp(t, k) for k in range(8)], -1).astype(f32)
    tin = np.concatenate([t[:, None], np.sin(q, dtype=f32), np.cos(q, dtype=f32)], -1).astype(f32)
    pre = np.broadcast_to(W["l1b"][None, :], (N, 64)).astype(f32)
    for i in range(17):
        pre = fma32(W["l1w"][None, :, i], tin[:, i:i + 1], pre)
    h = np.maximum(pre, f32(0.0))
    tout = np.broadcast_to(W["l2b"][None, :], (N, 30)).astype(f32)
    for k in range(64):
        tout = fma32(W["l2w"][None, :, k], h[:, k:k + 1], tout)
    out = dict(pre=pre, tout=tout)
    if dtout is None:
        return out
    dz2 = np.zeros((N, 30), dtype=f32)
    t0, t1, slot = ray_tiles(N, S)
    for n in range(N):
        if dtp is None or t0[n] == t1[n]:
            dz2[n] = dtout[n, :30]
        else:
            v = dtp[t0[n], slot[n], :30].astype(f32)
            for tl in range(t0[n] + 1, t1[n] + 1):
                v = (v + dtp[tl, 0, :30]).astype(f32)
            dz2[n] = v
    dh = np.zeros((N, 64), dtype=f32)
    for o in range(30):
        dh = fma32(W["l2w"][None, o, :], dz2[:, o:o + 1], dh)
    dz1 = np.where(pre > 0, dh, f32(0.0))

    def sums(a, b, key):   # [N][A], [N][B] -> pre_fill[key] + sum over the rays of a (x) b
        acc = np.asarray(pre_fill[key], dtype=f32).copy()
        for n0 in range(0, N, 32):
            blk = np.zeros((a.shape[1], b.shape[1]), dtype=f32)
            for n in range(n0, min(n0 + 32, N)):
                blk = fma32(a[n][:, None], b[n][None, :], blk)
            acc = (acc + blk.reshape(acc.shape)).astype(f32)
        return acc

    ones = np.ones((N, 1), dtype=f32)
    out.update(l2w=sums(dz2, h, "l2w"), l1w=sums(dz1, tin, "l1w"), l2b=sums(dz2, ones, "l2b"), l1b=sums(dz1, ones, "l1b"))
    return out
