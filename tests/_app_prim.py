"""Float64 references, seeded generators and derived bounds for the backward-data kernels of the appearance phase, shared by
test_app_primitives_cpu.py and test_gpu_app_primitives.py.  No GPU.
  * k_dyn_app_bwd<FEAT, REC> (dynamic field: MLP_Fea_late_view) and k_static_app_bwd<HEAD, FEAT> (static field: MLP_Fea |
    MLP_Fea_TimeEmbedding) behind rdrf_selftest_app_bwd, on saved rows, a compaction list and cotangents the test supplies.
The rows need not come from a forward pass: the kernels only read them, and the reference restates the chain from the same rows.
Every reference widens the float32 inputs to float64 and returns per output the value and an absolute bound k 2^-24 cond (+ what
the bounds of its inputs contribute), cond being the sum of the absolute values of the terms added and k the count of the kernel's
rounded operations on the way.  U = 2^-24.  An output whose cond is 0 has the bound 0 and must be exactly 0.  TINY = 2^-126 is added
per term that can fall below the smallest normal number (it may be flushed).  No constant was tuned against the kernels.

Layouts come from the library: rdrf_selftest_app_describe (rows of a tile, launch geometry), rdrf_selftest_dw_describe (the first
layer's column behind every saved input row, which is the column behind the same element of the backward-data result) and
rdrf_selftest_scatter_describe (the DA row and the record offset of every feature quad).  A vector's element e is row (first row + e).

Operation counts (k), in the order of the kernels:
  view direction v = d / |d| (ndc, contract): three products and two additions of positive terms (3), sqrt (1 + half of the 3),
      the division (1): K_VDIR = 4 relative; RDRF_RAY_OTHER takes d as it is: exact.
  logit v_o = W[o] H2 + b_o (+ Wv[o] vd): an fma chain of 64 per lane half, the sum of the halves, the bias, three view terms whose
      factor carries K_VDIR: K_LOGIT = 64 + 1 + 1 + 3 + 4 = 73 on cond = sum |W H2| + |b| + sum |Wv vd|.
  dzv = g r (1 - r): a logit error e moves ln(r (1 - r)) by |1 - 2 r| e <= e; r = 1 / (1 + expf(-v)) carries 6 U of itself (expf
      within 2 ulp = 4, the sum, the division: the allowance of tests/_heads_prim.py); 1 - r is a SUM of the terms 1 and r, so
      cond = |g| r (1 + r) and K_SIG = 6 + 3 (the difference, two products).  A saturated logit gives an r or a product below
      2^-126, which may be flushed: TINY (1 + |g|).
  dz2 = [H2 > 0] sum_o W[o][k] dzv_o: three fma, K_SMALL = 3.
  W^T dz products (layer 2, layer 1, basis): bf16 x 3 with split storage, held by tests/test_gpu_mlp_primitives.py as B3S_T; b3s_bound
      imports that file's two bounds as tests/_heads_prim.py does -- 2 e_seq32 of the same inputs and ONE_HOT_BOUND -- relative to
      sum |dz| |w|.
  x0_bwd: dq = ldexp(dS c - dC s, f) is two products and a difference (2), each coordinate sums its own element and ten dq over the
      two lane halves (11): K_X0 = 13.
  PE2 backward: dF += d0 c1 - d1 s1 + 2 (d2 c2 - d3 s2): products (1), the two differences (1), the factor 2 (exact), two
      additions (2): K_PE2 = 4.
  time-embedding view gradient w3^T dzv: three fma, K_SMALL.
  projection (g - (g.v) v) / |d|: g.v is three products and two additions on factors carrying K_VDIR (3 + 4 = 7); the product with
      v (1 + K_VDIR), the difference (1), |d| (2.5) and the division (1): K_PROJ = 10 (rounded up).
  g_rays: one atomic per sample of the ray in no fixed order: m additions onto the pre-fill, k = m on |pre| + sum |terms|."""
import ctypes as C

import numpy as np

import _dw_prim as DW
import _gather_prim as GP   # noqa: F401  (the sincos allowance is not needed: the kernels read saved sin / cos rows)
import _heads_prim as HP
import _mlp_prim as MP
import _scatter_prim as SC

f32, f64 = np.float32, np.float64
U, TINY, NAN = HP.U, HP.TINY, HP.NAN
ratio = HP.ratio
rows_of = HP.rows_of
K_VDIR, K_LOGIT, K_SIG, K_SMALL, K_X0, K_PE2, K_PROJ = 4, 73, 9, 3, 13, 4, 10
POWER = 16.0   # a planted defect must exceed the bound by this factor

FIELDS = {"dyn": 0, "fea": 1, "te": 2}
MODES = {"rows": 0, "rec": 1, "feat": 2}
RAY_TYPES = ("ndc", "contract", "world", "other")
COUNTS = (0, 1, 31, 32, 33, 95)
S_VALUES = (1, 13, 70)
GATES = np.array([0.0, -0.0, 2.0 ** -126, 1.0, -1.0, 0.37, -2.5], dtype=f32)
DEFECTS = {"pe2_factor": ("fea", "te"), "x0_swap": ("dyn",), "gate_ge": ("dyn", "fea", "te"), "view_in_dF": ("fea",),
           "no_projection": ("fea", "te"), "r_only": ("dyn", "fea", "te"), "rec_swap": ("dyn",), "no_view_cols": ("dyn", "te")}


def ray_type_id(L, name):
    return L.RAY_TYPES.get(name, 2)


# ---- layouts from the library --------------------------------------------------------------------------------------------------
def app_describe(L, field, mode, N, S=1):
    buf = (C.c_int * 16)()
    n = L.lib.rdrf_selftest_app_describe(FIELDS[field], MODES[mode], int(N), int(S), buf, 16)
    if n < 0:
        raise RuntimeError(f"rdrf_selftest_app_describe: rc {n}: {L.lib.rdrf_last_error().decode()}")
    assert buf[0] == n
    return dict(zip(("grid", "waves", "tiles", "rows", "grows", "DZV", "DZ2", "DZ1", "DF", "DA", "H2", "H1", "IN", "rec", "nda"), buf[1:n]))


def layout(L, field):
    """the describe of the field plus: fcol [32] / icol [64 | 128]: first-layer column behind each dF element and behind each
    element of the second input block (X0 or P; -1: padding), quads: per feature quad (first DA element, record offset or -1),
    unread: (first row, rows) of every saved block the ray path must not read, pw [128]: feature behind each P element (static)"""
    lay = app_describe(L, field, "rows", 1, 1)
    dyn = field == "dyn"
    plan = {"dyn": "DYN_APP", "fea": "STATIC_FEA", "te": "STATIC_TE"}[field]
    struct, wname = (L.RdrfDynamicParams, "rw1") if dyn else (L.RdrfStaticParams, "w1")
    js = [j for j in DW.describe(L, plan, 0)["jobs"] if j["w_off"] == getattr(struct, wname).offset]
    assert len(js) == 1 and js[0]["A_row0"] == lay["DZ1"] and js[0]["out_dim"] == 128
    col = {}
    for row0, cols in js[0]["blocks"]:
        for i, c in enumerate(cols):
            col[row0 + i] = int(c)
    f0 = [r for r, c in col.items() if c == 0]
    assert len(f0) == 1
    nin = 64 if dyn else 128
    lay["F"] = f0[0]
    lay["fcol"] = np.array([col.get(f0[0] + e, -1) for e in range(32)])
    lay["icol"] = np.array([col.get(lay["IN"] + e, -1) for e in range(nin)])
    lay["in_dim"] = js[0]["in_dim"]
    assert (lay["fcol"][:27] == np.arange(27)).all() and (lay["fcol"][30:] == -1).all()
    if dyn:
        lay["icol"][3] = -1   # the time column: computed by the kernel, used by nothing, never written
    else:
        e = np.arange(128)
        r, h, m = e >> 3, (e >> 2) & 1, e & 3
        lay["pw"] = 8 * (r >> 2) + 4 * h + (r & 3)
        base = 30 if field == "fea" else 27
        want = np.where(lay["pw"] < 27, base + np.where(m & 1, 54, 0) + 2 * lay["pw"] + (m >> 1), -1)
        assert (lay["icol"] == want).all(), "P rows: (sin f, cos f, sin 2f, cos 2f) of feature pw"
    sd = SC.describe(L, "DYN_APP" if dyn else "STATIC_APP")
    assert sd["row0"][0] == lay["DA"] and sd["rec_floats"] == lay["rec"] and 4 * sd["nq"] <= 2 * lay["nda"]
    lay["quads"] = [(q[0], q[4]) for q in sd["quads"]]
    lay["ncomp"] = 4 * sd["nq"]
    read = sorted([(lay["H2"], 128), (lay["H1"], 128), (lay["IN"], nin)])
    unread, at = [], 0
    for r0, n in read + [(lay["rows"], 0)]:
        if r0 > at:
            unread.append((at, r0 - at))
        at = r0 + n
    lay["unread"] = unread
    return lay


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def app_weights(field, seed=0, logit_bias=0.0):
    rng = np.random.default_rng([29, FIELDS[field], seed])
    n = lambda *s: rng.standard_normal(s, dtype=f32)   # noqa: E731
    in1 = {"dyn": 107, "fea": 138, "te": 135}[field]
    in3 = 128 if field == "fea" else 131
    nc = 216 if field == "dyn" else 72
    W = {"w1": n(128, in1) / f32(np.sqrt(in1)), "w2": n(128, 128) / f32(np.sqrt(128.0)), "w3": n(3, in3) / f32(np.sqrt(in3)),
         "b3": (n(3) * f32(0.1) + f32(logit_bias)).astype(f32), "basis": n(27, nc) / f32(np.sqrt(nc))}
    return {k: np.ascontiguousarray(v, dtype=f32) for k, v in W.items()}


def app_case(field, mode, N, S, count, ray_type="ndc", seed=0, g_channel=None, h2_scale=1.0):
    """ray path: `count` distinct samples of [N][S] in random order; feature mode: N points (S, count ignored).  Saved rows: H2 and
    H1 draw from GATES and normal values, the second input block from [-1, 1]; every lane of the tiles the kernel walks is finite,
    the padding lanes included"""
    rng = np.random.default_rng([31, FIELDS[field], MODES[mode], N, S, count, seed])
    c = dict(field=field, mode=mode, N=N, S=S, ray_type=ray_type, seed=seed)
    if mode == "feat":
        c.update(count=N, n=N, g_feat=rng.standard_normal((N, 27), dtype=f32))
        return c
    ns = N * S
    assert 0 <= count <= ns
    T = (count + 31) // 32
    lst = np.full(ns, 0x7fffffff, dtype=np.int32)
    lst[:count] = rng.permutation(ns)[:count].astype(np.int32)

    def gates(shape):
        pick = rng.integers(0, len(GATES) + 3, size=shape)
        return np.where(pick < len(GATES), GATES[np.minimum(pick, len(GATES) - 1)], rng.standard_normal(shape, dtype=f32)).astype(f32)

    nin = 64 if field == "dyn" else 128
    rays = np.concatenate([rng.standard_normal((N, 3), dtype=f32), rng.standard_normal((N, 3), dtype=f32) * f32(1.7) + f32(0.2)], 1)
    g = rng.standard_normal((ns, 3), dtype=f32)
    if g_channel is not None:
        g[:, [o for o in range(3) if o != g_channel]] = 0
    c.update(count=count, n=count, T=T, list=lst, rays=np.ascontiguousarray(rays, dtype=f32), g_rgb=g,
             H2=(gates((T * 32, 128)) * f32(h2_scale)).astype(f32), H1=gates((T * 32, 128)),
             IN=rng.uniform(-1.0, 1.0, (T * 32, nin)).astype(f32))
    return c


def app_rows(c, lay, poison=True):
    """act3 [tiles of N S][rows][32]: the rows the kernel reads in the tiles it walks, NaN everywhere else (poison) or zeros"""
    tiles = (c["N"] * c["S"] + 31) // 32
    a = np.full((tiles, lay["rows"], 32), NAN if poison else 0.0, dtype=f32)
    T = c["T"]
    for key, n in (("H2", 128), ("H1", 128), ("IN", c["IN"].shape[1])):
        a[:T, lay[key]:lay[key] + n, :] = c[key].reshape(T, 32, n).transpose(0, 2, 1)
    return a


# ---- reference -----------------------------------------------------------------------------------------------------------------
def _sigmoid(x):
    return HP._sigmoid(x)


def b3s_bound(x32, We):
    """relative bound (of sum |x| |w|) of a split-storage bf16 x 3 product: the two bounds tests/test_gpu_mlp_primitives.py holds
    the B3S_T forms to, added, as tests/_heads_prim.py b3_pair_bound does"""
    return 2.0 * MP.e_seq32(np.ascontiguousarray(x32, dtype=f32), np.ascontiguousarray(We, dtype=f32)) + MP.ONE_HOT_BOUND


def _weff(w, cols):
    """[len(cols)][out]: row e is column cols[e] of w [out][in] (zeros where cols[e] < 0)"""
    return np.where(cols[:, None] >= 0, np.asarray(w, dtype=f64)[:, np.maximum(cols, 0)].T, 0.0)


def _product(x, bx, We):
    """y = x We^T with its bound: b3s_bound cond + |We| bx (+ TINY where anything is summed)"""
    y, cond = x @ We.T, np.abs(x) @ np.abs(We).T
    rel = b3s_bound(x.astype(f32), We.astype(f32)) if x.size else 0.0
    return y, bx @ np.abs(We).T + rel * cond + TINY * (cond > 0)


def view_dirs(c, n_of):
    """-> v [n][3], |d| [n], relative error units of v"""
    d = np.asarray(c["rays"], dtype=f64)[n_of, 3:6]
    if c["ray_type"] in ("ndc", "contract"):
        nr = np.sqrt((d * d).sum(1))
        return d / nr[:, None], nr, K_VDIR
    return d, np.ones(len(d)), 0


def app_reference(c, W, lay, defect=None, pre_rays=None):
    """-> {name: (value, bound)} per compacted sample (feature mode: per point): 'dzv' [n][3], 'dz2', 'dz1' [n][128], 'dF' [n][32],
    'dA' [n][2 nda], dynamic: 'dxn' [n][3] and with records 'rec' [n][216]; static: 'g_rays' [N][3] (onto pre_rays [N][3])"""
    field, n = c["field"], c["n"]
    dyn = field == "dyn"
    out = {}
    basis = np.asarray(W["basis"], dtype=f64)   # [27][ncomp]
    Wb = np.zeros((2 * lay["nda"], 32))
    Wb[:lay["ncomp"], :27] = basis.T
    if c["mode"] == "feat":
        dF = np.zeros((n, 32))
        dF[:, :27] = np.asarray(c["g_feat"], dtype=f64)
        out["dF"] = (dF, np.zeros_like(dF))
        out["dA"] = _product(dF, np.zeros_like(dF), Wb)
        return out
    idx = c["list"][:n].astype(np.int64)
    n_of = idx // c["S"]
    H2, H1, IN = (np.asarray(c[k][:n], dtype=f64) for k in ("H2", "H1", "IN"))
    g = np.asarray(c["g_rgb"], dtype=f64)[idx] if c["g_rgb"] is not None else np.zeros((n, 3))
    w3, b3 = np.asarray(W["w3"], dtype=f64), np.asarray(W["b3"], dtype=f64)
    vd, nr, kv = view_dirs(c, n_of)
    # ---- output layer
    v = H2 @ w3[:, :128].T + b3
    condv = np.abs(H2) @ np.abs(w3[:, :128]).T + np.abs(b3)
    if field != "fea" and defect != "no_view_cols":
        v = v + vd @ w3[:, 128:131].T
        condv = condv + np.abs(vd) @ np.abs(w3[:, 128:131]).T
    ev = K_LOGIT * U * condv + 128 * TINY
    r = _sigmoid(v)
    dzv = g * r if defect == "r_only" else g * r * (1.0 - r)
    bzv = (K_SIG * U + ev) * np.abs(g) * r * (1.0 + r) + TINY * (1.0 + np.abs(g)) * (g != 0)
    out["dzv"] = (dzv, bzv)
    gate = (lambda H: H >= 0) if defect == "gate_ge" else (lambda H: H > 0)
    # ---- dz2
    W3h = w3[:, :128]
    t2, c2 = dzv @ W3h, np.abs(dzv) @ np.abs(W3h)
    dz2 = np.where(gate(H2), t2, 0.0)
    bz2 = np.where(gate(H2), bzv @ np.abs(W3h) + K_SMALL * U * c2 + TINY * (c2 > 0), 0.0)
    out["dz2"] = (dz2, bz2)
    # ---- layer 2
    y1, by1 = _product(dz2, bz2, np.asarray(W["w2"], dtype=f64).T)
    dz1, bz1 = np.where(gate(H1), y1, 0.0), np.where(gate(H1), by1, 0.0)
    out["dz1"] = (dz1, bz1)
    # ---- layer 1: the feature block and the second input block in one product
    cols = np.concatenate([lay["fcol"], lay["icol"]])
    Y, bY = _product(dz1, bz1, _weff(W["w1"], cols))
    dF, bF, dI, bI = Y[:, :32].copy(), bY[:, :32].copy(), Y[:, 32:], bY[:, 32:]
    if dyn:
        dxn, cxn, bxn = dI[:, :3].copy(), np.abs(dI[:, :3]), bI[:, :3].copy()
        for j in range(30):
            e = 4 + 4 * (j >> 1) + 2 * (j & 1)
            d, f = j // 10, 2.0 ** (j % 10)
            sv_, cv_ = (IN[:, e + 1], IN[:, e]) if defect == "x0_swap" else (IN[:, e], IN[:, e + 1])
            dxn[:, d] += f * (dI[:, e] * cv_ - dI[:, e + 1] * sv_)
            cxn[:, d] += f * (np.abs(dI[:, e] * cv_) + np.abs(dI[:, e + 1] * sv_))
            bxn[:, d] += f * (bI[:, e] * np.abs(cv_) + bI[:, e + 1] * np.abs(sv_))
        out["dxn"] = (dxn, bxn + K_X0 * U * cxn + TINY * (cxn > 0))
    else:
        two = 1.0 if defect == "pe2_factor" else 2.0
        for e0 in range(0, 128, 4):
            w = lay["pw"][e0]
            d, bd, P = dI[:, e0:e0 + 4], bI[:, e0:e0 + 4], IN[:, e0:e0 + 4]
            terms = np.stack([d[:, 0] * P[:, 1], -d[:, 1] * P[:, 0], two * d[:, 2] * P[:, 3], -two * d[:, 3] * P[:, 2]], 1)
            bt = bd[:, 0] * np.abs(P[:, 1]) + bd[:, 1] * np.abs(P[:, 0]) + 2.0 * (bd[:, 2] * np.abs(P[:, 3]) + bd[:, 3] * np.abs(P[:, 2]))
            cond = np.abs(dF[:, w]) + np.abs(terms).sum(1)
            dF[:, w] += terms.sum(1)
            bF[:, w] += bt + K_PE2 * U * cond + TINY * (np.abs(terms).sum(1) > 0)
        # ---- the view-direction gradient
        if field == "fea":
            gv, bgv = dF[:, 27:30].copy(), bF[:, 27:30].copy()
            if defect != "view_in_dF":
                dF[:, 27:30], bF[:, 27:30] = 0.0, 0.0
        else:
            Wv = w3[:, 128:131]
            gv, cgv = dzv @ Wv, np.abs(dzv) @ np.abs(Wv)
            bgv = bzv @ np.abs(Wv) + K_SMALL * U * cgv + TINY * (cgv > 0)
        if c["ray_type"] in ("ndc", "contract") and defect != "no_projection":
            dot, cdot = (gv * vd).sum(1), np.abs(gv * vd).sum(1)
            bdot = (bgv * np.abs(vd)).sum(1) + (3 + kv) * U * cdot
            contrib = (gv - dot[:, None] * vd) / nr[:, None]
            ccon = (np.abs(gv) + np.abs(dot[:, None] * vd)) / nr[:, None]
            bcon = (bgv + bdot[:, None] * np.abs(vd)) / nr[:, None] + K_PROJ * U * ccon + TINY * (ccon > 0)
        else:
            contrib, ccon, bcon = gv, np.abs(gv), bgv
        pre = np.zeros((c["N"], 3)) if pre_rays is None else np.asarray(pre_rays, dtype=f64)
        tot, ctot, btot, m = pre.copy(), np.abs(pre), np.zeros_like(pre), np.zeros(c["N"])
        np.add.at(tot, n_of, contrib)
        np.add.at(ctot, n_of, ccon)
        np.add.at(btot, n_of, bcon)
        np.add.at(m, n_of, 1.0)
        out["g_rays"] = (tot, btot + m[:, None] * U * ctot)
        out["g_rays_terms"] = (contrib, bcon)
    out["dF"] = (dF, bF)
    out["dA"] = _product(dF, bF, Wb)
    if c["mode"] == "rec":
        dA, bA = out["dA"]
        rec, brec = np.zeros((n, lay["rec"])), np.zeros((n, lay["rec"]))
        quads = list(lay["quads"])
        if defect == "rec_swap":
            quads[14], quads[15] = (quads[14][0], quads[15][1]), (quads[15][0], quads[14][1])
        for e0, off in quads:
            rec[:, off:off + 4], brec[:, off:off + 4] = dA[:, e0:e0 + 4], bA[:, e0:e0 + 4]
        out["rec"] = (rec, brec)
    return out


# ---- the same chains in float32, in the kernels' order ---------------------------------------------------------------------------
def _prod32(x, We):
    """a bf16 x 3 product: the six piece products of tests/_mlp_prim.py summed, rounded to float32"""
    return MP.emulate_b3(np.ascontiguousarray(x, dtype=f32), np.ascontiguousarray(We, dtype=f32)).astype(f32)


def app_eval32(c, W, lay, pre_rays=None):
    field, n = c["field"], c["n"]
    dyn = field == "dyn"
    out = {}
    Wb = np.zeros((2 * lay["nda"], 32), dtype=f32)
    Wb[:lay["ncomp"], :27] = W["basis"].T
    one, zero = f32(1.0), f32(0.0)
    if c["mode"] == "feat":
        dF = np.zeros((n, 32), dtype=f32)
        dF[:, :27] = c["g_feat"]
        out["dF"], out["dA"] = dF, _prod32(dF, Wb)
        return out
    idx = c["list"][:n].astype(np.int64)
    n_of = idx // c["S"]
    H2, H1, IN = c["H2"][:n], c["H1"][:n], c["IN"][:n]
    g = c["g_rgb"][idx] if c["g_rgb"] is not None else np.zeros((n, 3), dtype=f32)
    w3, b3 = W["w3"], W["b3"]
    d = c["rays"][n_of, 3:6]
    if c["ray_type"] in ("ndc", "contract"):
        nr = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
        vd = (d / nr[:, None]).astype(f32)
    else:
        nr, vd = np.ones(n, dtype=f32), d
    half = ((np.arange(128) >> 2) & 1).astype(bool)   # the elements each lane half holds: an fma chain per half, then their sum
    v = (MP.seq32(H2[:, ~half].copy(), w3[:, :128][:, ~half].copy()) + MP.seq32(H2[:, half].copy(), w3[:, :128][:, half].copy())) + b3
    if field != "fea":
        for i in range(3):
            v = v + w3[None, :, 128 + i] * vd[:, i:i + 1]
    with np.errstate(over="ignore"):
        r = one / (one + np.exp(-v, dtype=f32))
    dzv = (g * r * (one - r)).astype(f32)
    out["dzv"] = dzv
    t2 = MP.seq32(dzv, w3[:, :128].T.copy())
    dz2 = np.where(H2 > 0, t2, zero)
    dz1 = np.where(H1 > 0, _prod32(dz2, W["w2"].T), zero)
    out["dz2"], out["dz1"] = dz2, dz1
    cols = np.concatenate([lay["fcol"], lay["icol"]])
    Y = _prod32(dz1, _weff(W["w1"], cols).astype(f32))
    dF, dI = Y[:, :32].copy(), Y[:, 32:]
    assert dF.dtype == f32 and dz1.dtype == f32
    if dyn:
        dxn = dI[:, :3].copy()
        for j in range(30):
            e = 4 + 4 * (j >> 1) + 2 * (j & 1)
            dq = (dI[:, e] * IN[:, e + 1] - dI[:, e + 1] * IN[:, e]) * f32(2.0 ** (j % 10))
            dxn[:, j // 10] = dxn[:, j // 10] + dq
        out["dxn"] = dxn
    else:
        for e0 in range(0, 128, 4):
            w = lay["pw"][e0]
            dd, P = dI[:, e0:e0 + 4], IN[:, e0:e0 + 4]
            dF[:, w] = dF[:, w] + ((dd[:, 0] * P[:, 1] - dd[:, 1] * P[:, 0]) + f32(2.0) * (dd[:, 2] * P[:, 3] - dd[:, 3] * P[:, 2]))
        if field == "fea":
            gv = dF[:, 27:30].copy()
            dF[:, 27:30] = zero
        else:
            gv = MP.seq32(dzv, w3[:, 128:131].T.copy())
        if c["ray_type"] in ("ndc", "contract"):
            dot = gv[:, 0] * vd[:, 0] + gv[:, 1] * vd[:, 1] + gv[:, 2] * vd[:, 2]
            contrib = ((gv - dot[:, None] * vd) / nr[:, None]).astype(f32)
        else:
            contrib = gv
        tot = (np.zeros((c["N"], 3)) if pre_rays is None else np.asarray(pre_rays)).astype(f32)
        for i in range(n):
            tot[n_of[i]] = tot[n_of[i]] + contrib[i]
        assert tot.dtype == f32
        out["g_rays"] = tot
    out["dF"], out["dA"] = dF, _prod32(dF, Wb)
    if c["mode"] == "rec":
        rec = np.zeros((n, lay["rec"]), dtype=f32)
        for e0, off in lay["quads"]:
            rec[:, off:off + 4] = out["dA"][:, e0:e0 + 4]
        out["rec"] = rec
    return out


def compared(c):
    """the outputs of a case that carry a bound"""
    if c["mode"] == "feat":
        return ("dF", "dA")
    names = ["dzv", "dz2", "dz1", "dF", "dA"]
    names += ["dxn"] if c["field"] == "dyn" else ["g_rays"]
    if c["mode"] == "rec":
        names[names.index("dA")] = "rec"
    return tuple(names)


def cpu_cases():
    """the generated cases of the CPU file: every field, mode and ray type at every small count, S from S_VALUES"""
    out = []
    for fi, field in enumerate(FIELDS):
        for ci, count in enumerate(COUNTS):
            S = S_VALUES[(ci + fi) % 3]
            N = max(1, -(-(count + 9) // S))
            for mode in (("rows", "rec") if field == "dyn" else ("rows",)):
                for rt in (RAY_TYPES if field != "dyn" else ("ndc", "other")):
                    out.append(app_case(field, mode, N, S, count, rt, seed=ci))
        for M in (1, 33, 70):
            out.append(app_case(field, "feat", M, 1, M))
    return out


def large_tiles(L, field, limit=2050):
    """(the smallest tile count whose launch has several waves per workgroup, the smallest at which the workgroups' queues hand
    out a second round: more tiles than waves in the launch), read from rdrf_selftest_app_describe"""
    t_waves = t_walk = None
    for t in range(1, limit + 1):
        g = app_describe(L, field, "rows", t * 32, 1)
        if t_waves is None and g["waves"] > 1:
            t_waves = t
        if t_walk is None and g["waves"] > 1 and t > g["grid"] * g["waves"]:
            t_walk = t
            break
    assert t_waves is not None and t_walk is not None
    return t_waves, t_walk
