"""rdrf_scene_flow_bwd with the weight gradients formed in the backward-data kernel (csrc/rdrf_bwd_fused.hip k_scene_flow_bwd_dw)
on activation rows the test supplies (`saved` is an input of the entry point: [tile][256 rows][32 samples], X | H0 | H2 | H4).

The reference is the layer equations alone, per sample n (dz6 = [g_f, g_b], zero where a gradient is absent):
    dz4 = [H4 > 0] W3^T dz6,  dz2 = [H2 > 0] W2^T dz4,  dz0 = [H0 > 0] W1^T dz2,
    dW3 = sum dz6 (x) H4,  dW2 = sum dz4 (x) H2,  dW1 = sum dz2 (x) H0,  dW0[:, col(e)] = sum dz0 X[e],  db_l = sum dz_l,
col(e) being the slot order of the first layer's input rows as rdrf_selftest_dw_describe reports it for the scene-flow plan.

(a) exact: weights in {-1, 0, 1} with two non-zeros per input column, upstream gradients in {-1, 0, 1}, rows in [-2, 2]: every
    dz is an integer of at most 8 and every partial sum stays below 2^24 (the bound is computed from the case), so no order of
    accumulation can change a bit: torch.equal with the int64 sums, on integer pre-filled gradients, at sample counts around
    the tile edge, with fewer tiles than waves, with a nearly empty last workgroup and with grid * waves + 3 tiles (some
    waves walk a second tile; grid and waves come from rdrf_selftest_sf_geometry, the helper the launch uses); with the point
    gradient absent and with only one of the two upstream gradients.  g_pts of the same runs, onto its zero pre-fill, is
    fl32(e inv32) bit for bit, e the exact gradient of the normalised point from the float64 reference of tests/_warp_prim.py
    (the harness's box has no power-of-two inv: one rounding, contracted or not).  Dense inputs: tests/test_gpu_warp_primitives.py.
(b) accuracy: dense normal rows and weights at 257 tiles, e = max |dW - dW64| / sum |dz| |in| within 2 x e_seq32, the same
    metric of an fp32 evaluation that sums the samples sequentially (the form tests/test_gpu_dw_primitives.py (c) holds k_dw3 to).
(c) poison: 3e38 in every activation slot of the samples whose upstream gradient is zero and of the slots past N * S changes
    no bit of any output; nor does a workspace pre-filled with 0xFF bytes against a zeroed one.
(d) the tools build (RDRF_SF_FUSED, read once per process: one child per setting): the fused kernel against k_scene_flow_bwd +
    k_dw3 -- identical on the exact inputs, both within the bound of (b) on the dense ones, g_pts bit-identical in both.
The int64 / float64 side is checked against plain loops without a GPU (test_reference_against_plain_loops)."""
import ctypes as C

import numpy as np
import pytest
import torch

from _twin import CHILD, run_twin, tools_lib
from _util import pkg, profile_line

ROWS, R_X, R_H0, R_H2, R_H4 = 256, 0, 64, 128, 192
SHAPES = [(64, 36), (64, 64), (64, 64), (6, 64)]   # scene_flow_mlp.{0,2,4,6}.weight
PREFILL = 3
DENSE_TILES = 257
GUARD = 64   # floats of NaN on either side of g_pts
BOX = [[-1.5, -1.67, -1.0], [1.5, 1.67, 1.0]]   # the harness's own box: no inv is a power of two


def _x_cols():
    """element (row of the X block) -> column of scene_flow_mlp.0.weight, -1: padding; from the scene-flow plan's description"""
    import _dw_prim as P
    desc = P.describe(pkg(), "SCENE_FLOW", 0)
    job = [j for j in desc["jobs"] if j["in_dim"] == 36]
    assert len(job) == 1
    cols = np.full(64, -1, dtype=np.int64)
    for row0, c in job[0]["blocks"]:
        cols[row0 - R_X:row0 - R_X + 32] = c
    assert sorted(cols[cols >= 0]) == list(range(36))
    return cols


def geometry(ntiles):
    L = pkg()
    g, w = C.c_int(0), C.c_int(0)
    L.check(L.lib.rdrf_selftest_sf_geometry(int(ntiles), C.byref(g), C.byref(w)), "rdrf_selftest_sf_geometry")
    return g.value, w.value


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def int_case(n, seed):
    """rows [T][256][32] (every slot, the ones past n included), weights, upstream gradients: small integers"""
    rng = np.random.default_rng([7, seed, n])
    T = (n + 31) // 32
    rows = rng.integers(-2, 3, size=(T, ROWS, 32)).astype(np.float32)
    W = []
    for out, inn in SHAPES:
        w = np.zeros((out, inn), dtype=np.float32)
        for k in range(inn):
            w[rng.choice(out, size=2, replace=False), k] = rng.choice([-1.0, 1.0], size=2)
        W.append(w)
    gf = rng.integers(-1, 2, size=(n, 3)).astype(np.float32)
    gb = rng.integers(-1, 2, size=(n, 3)).astype(np.float32)
    return rows, W, gf, gb


def dense_case(seed, T=DENSE_TILES):
    rng = np.random.default_rng([11, seed])
    n = T * 32 - 5
    rows = rng.standard_normal((T, ROWS, 32), dtype=np.float32)
    W = [(rng.standard_normal(s, dtype=np.float32) / np.float32(np.sqrt(s[1]))) for s in SHAPES]
    gf = rng.standard_normal((n, 3), dtype=np.float32)
    gb = rng.standard_normal((n, 3), dtype=np.float32)
    return n, rows, W, gf, gb


# ---- reference ------------------------------------------------------------------------------------------------------------
def _chain(rows, W, gf, gb, n, dtype):
    """per-sample layer inputs and dz of every layer: [(dz, input)] for layers 0..3, X already in weight-column order"""
    T = rows.shape[0]
    a = rows.transpose(0, 2, 1).reshape(T * 32, ROWS)[:n].astype(dtype)
    W = [w.astype(dtype) for w in W]
    dz6 = np.zeros((n, 6), dtype=dtype)
    if gf is not None:
        dz6[:, :3] = gf
    if gb is not None:
        dz6[:, 3:] = gb
    X, H0, H2, H4 = a[:, R_X:R_X + 64], a[:, R_H0:R_H0 + 64], a[:, R_H2:R_H2 + 64], a[:, R_H4:R_H4 + 64]
    dz4 = np.where(H4 > 0, dz6 @ W[3], 0).astype(dtype)
    dz2 = np.where(H2 > 0, dz4 @ W[2], 0).astype(dtype)
    dz0 = np.where(H0 > 0, dz2 @ W[1], 0).astype(dtype)
    cols = _x_cols()
    Xc = np.zeros((n, 36), dtype=dtype)
    Xc[:, cols[cols >= 0]] = X[:, cols >= 0]
    return [(dz0, Xc), (dz2, H0), (dz4, H2), (dz6, H4)]


def reference(rows, W, gf, gb, n, absolute=False):
    """float64 (exact for the integer cases: every sum is an integer far below 2^53): [dW0..3], [db0..3]"""
    ch = _chain(rows, W, gf, gb, n, np.float64)
    if absolute:
        ch = [(np.abs(d), np.abs(i)) for d, i in ch]
    return [d.T @ i for d, i in ch], [d.sum(axis=0) for d, _ in ch]


def reference_loops(rows, W, gf, gb, n):
    """the same equations as plain int64 loops over samples and neurons (integer cases)"""
    cols = _x_cols()
    Wi = [w.astype(np.int64) for w in W]
    dW = [np.zeros(s, dtype=np.int64) for s in SHAPES]
    db = [np.zeros(s[0], dtype=np.int64) for s in SHAPES]
    for i in range(n):
        t, s = divmod(i, 32)
        col = rows[t, :, s].astype(np.int64)
        dz = np.zeros(6, dtype=np.int64)
        if gf is not None:
            dz[:3] = gf[i]
        if gb is not None:
            dz[3:] = gb[i]
        for layer, r0 in ((3, R_H4), (2, R_H2), (1, R_H0), (0, R_X)):
            out, inn = SHAPES[layer]
            for o in range(out):
                db[layer][o] += dz[o]
                for e in range(64):
                    c = e if layer else cols[e]
                    if c >= 0:
                        dW[layer][o, c] += dz[o] * col[r0 + e]
            if layer:
                nxt = np.zeros(64, dtype=np.int64)
                for k in range(64):
                    if col[r0 + k] > 0:
                        nxt[k] = sum(Wi[layer][o, k] * dz[o] for o in range(out))
                dz = nxt
    return dW, db


def e_seq32(rows, W, gf, gb, n, ref):
    """error metric of an fp32 evaluation of the same terms, the samples summed one after the other"""
    ch = _chain(rows, W, gf, gb, n, np.float32)
    mag = reference(rows, W, gf, gb, n, absolute=True)
    worst = 0.0
    for layer, (d, i) in enumerate(ch):
        acc = np.zeros(SHAPES[layer], dtype=np.float32)
        bias = np.zeros(SHAPES[layer][0], dtype=np.float32)
        tmp = np.empty_like(acc)
        for s in range(n):
            np.multiply(d[s][:, None], i[s][None, :], out=tmp)
            acc += tmp
            bias += d[s]
        worst = max(worst, float((np.abs(acc - ref[0][layer]) / mag[0][layer]).max()),
                    float((np.abs(bias - ref[1][layer]) / mag[1][layer]).max()))
    return worst


def metric(got, ref, mag):
    return max(max(float((np.abs(g.astype(np.float64) - r) / m).max()) for g, r, m in zip(got[k], ref[k], mag[k])) for k in (0, 1))


# ---- the call -------------------------------------------------------------------------------------------------------------
class Harness:
    """a small dynamic field for the parameter struct (the backward packs every weight of the field), scene-flow weights and
    gradient buffers of the test's own"""

    def __init__(self):
        import rodynrf
        from _gpu_util import COMMON
        self.L = pkg()
        self.F = pkg("fields")
        aabb = torch.tensor(BOX)
        kw = dict(COMMON, near_far=[0.0, 1.0], density_shift=-10.0, fea2denseAct="relu")
        torch.manual_seed(3)
        self.dy = rodynrf.TensorVMSplit_TimeEmbedding(aabb, [24, 26, 16], 12, "cuda:0", shadingMode="MLP_Fea_late_view", fea_pe=0, **kw)
        self.params = [p.detach() for p in self.dy._param_list()]
        self.cfg = self.F._cfg_struct(self.dy, "ndc")

    def cfg_for(self, box):
        """the field's configuration on another box [[lo 3], [hi 3]] (None: the harness's own, BOX)"""
        if box is None:
            return self.cfg
        cfg = type(self.cfg).from_buffer_copy(self.cfg)
        for i, v in enumerate(np.asarray(box, dtype=np.float32).reshape(6)):
            cfg.aabb[i] = float(v)
        return cfg

    def run(self, n, rows, W, gf, gb, pts=True, ws_byte=None, prefill=True, box=None, pts_fill=None):
        """-> ([dW0..3], [db0..3], g_pts or None) as numpy; gradients pre-filled with small integers (added into).  g_pts (pre-filled
        with pts_fill [n][3], else zeros) sits between NaN-poisoned guard bands of GUARD floats; self.guards_intact tells whether
        the last call left them alone, self.pts_buffer is the buffer after the call (untouched when the kernel got no g_pts)"""
        L, dev = self.L, "cuda:0"
        N, S = n, 1
        cfg = self.cfg_for(box)
        params = list(self.params)
        biases = [torch.zeros(s[0], device=dev) for s in SHAPES]
        for i in range(4):
            params[43 + 2 * i] = torch.from_numpy(W[i]).to(dev).contiguous()
            params[44 + 2 * i] = biases[i]
        P = self.F._dynamic_struct(params)
        rng = np.random.default_rng(5)
        pre_w = [rng.integers(-PREFILL, PREFILL + 1, size=s).astype(np.float32) if prefill else np.zeros(s, np.float32) for s in SHAPES]
        pre_b = [rng.integers(-PREFILL, PREFILL + 1, size=s[0]).astype(np.float32) if prefill else np.zeros(s[0], np.float32) for s in SHAPES]
        gw = [torch.from_numpy(a).to(dev) for a in pre_w]
        gbias = [torch.from_numpy(a).to(dev) for a in pre_b]
        grads = list(self.params)   # (addresses only: the scene-flow backward writes the eight scene-flow gradients)
        for i in range(4):
            grads[43 + 2 * i], grads[44 + 2 * i] = gw[i], gbias[i]
        G = self.F._dynamic_struct(grads)
        saved = torch.from_numpy(rows).to(dev).contiguous()
        assert saved.numel() == ((n + 31) // 32) * ROWS * 32
        xyz = torch.zeros(N, S, 3, device=dev)
        ts = torch.zeros(N, device=dev)
        band = torch.full((GUARD + n * 3 + GUARD,), float("nan"), device=dev)
        pbuf = band[GUARD:GUARD + n * 3].view(N, S, 3).zero_()
        if pts_fill is not None:
            pbuf.copy_(torch.from_numpy(np.ascontiguousarray(pts_fill, dtype=np.float32)).view(N, S, 3))
        g_pts = pbuf if pts else None
        cgf = None if gf is None else torch.from_numpy(gf).to(dev).contiguous()
        cgb = None if gb is None else torch.from_numpy(gb).to(dev).contiguous()
        nbytes = L.lib.rdrf_workspace_bytes(N, S)
        ws = torch.full((nbytes,), 0 if ws_byte is None else ws_byte, dtype=torch.uint8, device=dev)
        L.check(L.lib.rdrf_scene_flow_bwd(C.byref(P), C.byref(cfg), L.ptr(xyz), L.ptr(ts), N, S, L.ptr(cgf), L.ptr(cgb), C.byref(G),
                                          L.ptr(g_pts), L.ptr(saved), C.c_size_t(saved.numel() * 4), L.ptr(ws), C.c_size_t(ws.numel()),
                                          L.stream_of(saved)), "rdrf_scene_flow_bwd")
        torch.cuda.synchronize()
        self.guards_intact = bool(torch.isnan(torch.cat([band[:GUARD], band[-GUARD:]])).all())
        self.pts_buffer = pbuf.cpu().numpy().reshape(n, 3)
        dW = [g.cpu().numpy() for g in gw]
        db = [g.cpu().numpy() for g in gbias]
        return dW, db, (None if g_pts is None else g_pts.cpu().numpy()), pre_w, pre_b


_H = []


def _harness():
    if not _H:
        _H.append(Harness())
    return _H[0]


def exact_counts():
    grid, waves = geometry(1 << 20)
    big = grid * waves + 3
    assert geometry(big) == (grid, waves)
    return [1, 31, 32, 33, 5 * 32, 8 * 32 + 1, waves * 32 + 1, 32 * big]


def check_exact(run, n, seed, gf_on=True, gb_on=True, pts=True):
    rows, W, gf, gb = int_case(n, seed)
    gf, gb = (gf if gf_on else None), (gb if gb_on else None)
    ref = reference(rows, W, gf, gb, n)
    mag = reference(rows, W, gf, gb, n, absolute=True)
    bound = PREFILL + max(float(m.max()) for k in (0, 1) for m in mag[k])
    assert bound < 2 ** 24, bound   # any order of accumulation is exact
    dW, db, g_pts, pre_w, pre_b = run(n, rows, W, gf, gb, pts=pts)
    for layer in range(4):
        want_w = torch.from_numpy(np.rint(ref[0][layer]).astype(np.int64) + pre_w[layer].astype(np.int64))
        want_b = torch.from_numpy(np.rint(ref[1][layer]).astype(np.int64) + pre_b[layer].astype(np.int64))
        got_w, got_b = torch.from_numpy(dW[layer]), torch.from_numpy(db[layer])
        assert torch.equal(got_w.to(torch.int64), want_w) and torch.equal(got_w, want_w.float()), \
            f"n = {n}: dW of layer {layer}: {int((got_w != want_w.float()).sum())} entries differ"
        assert torch.equal(got_b.to(torch.int64), want_b) and torch.equal(got_b, want_b.float()), \
            f"n = {n}: db of layer {layer}: {int((got_b != want_b.float()).sum())} entries differ"
    assert (g_pts is None) == (not pts)
    if g_pts is not None:
        # against the float64 reference of tests/_warp_prim.py: on integers the gradient e of the normalised point is exact (the
        # guard asserts every partial sum below 2^24) and, onto the zero pre-fill, g_pts = fl32(e inv32): one rounding, the same
        # whether the product is contracted into the addition or not
        import _warp_prim as Q
        lay = Q.sf_layout(pkg())
        cq = dict(n=n, rows=rows, W=W, gf=gf, gb=gb, pre=np.zeros((n, 3), dtype=np.float32), box=np.asarray(BOX, dtype=np.float32))
        Q.sf_exact_guard(cq, lay)
        e = Q.sf_reference(cq, lay)["e"][0]
        want = e.astype(np.float32) * Q.box_inv(cq["box"])[None, :]
        assert np.array_equal(e, np.rint(e)) and want.dtype == np.float32
        assert np.array_equal(g_pts.reshape(n, 3).view(np.uint32), (want + np.float32(0.0)).view(np.uint32)), f"n = {n}: g_pts differs"
    return dW, db, g_pts


# ---- no GPU: the reference against plain loops ------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,n", [("both", 34), ("f", 5), ("b", 5)])
def test_reference_against_plain_loops(variant, n):
    rows, W, gf, gb = int_case(n, 1)
    gf, gb = (gf if variant != "b" else None), (gb if variant != "f" else None)
    ref = reference(rows, W, gf, gb, n)
    dW, db = reference_loops(rows, W, gf, gb, n)
    for layer in range(4):
        assert np.array_equal(np.rint(ref[0][layer]).astype(np.int64), dW[layer]) and np.array_equal(ref[0][layer], dW[layer].astype(np.float64))
        assert np.array_equal(np.rint(ref[1][layer]).astype(np.int64), db[layer])
    assert any(np.abs(d).max() > 0 for d in dW)
    mag = reference(rows, W, gf, gb, n, absolute=True)
    assert all((m >= np.abs(r)).all() for m, r in zip(mag[0], ref[0]))


# ---- (a) ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_exact_weight_gradients():
    H = _harness()
    counts = exact_counts()
    for n in counts:
        check_exact(H.run, n, 0)
    for n in counts[:-1]:
        check_exact(H.run, n, 1, pts=False)
        check_exact(H.run, n, 2, gb_on=False)
        check_exact(H.run, n, 3, gf_on=False)
    check_exact(H.run, counts[-1], 4, gb_on=False, pts=False)


# ---- (b) ------------------------------------------------------------------------------------------------------------------
def dense_reference(seed=0):
    n, rows, W, gf, gb = dense_case(seed)
    ref = reference(rows, W, gf, gb, n)
    mag = reference(rows, W, gf, gb, n, absolute=True)
    return (n, rows, W, gf, gb), ref, mag, e_seq32(rows, W, gf, gb, n, ref)


_DENSE = []


def _dense():
    if not _DENSE:
        _DENSE.append(dense_reference())
    return _DENSE[0]


@pytest.mark.gpu
def test_dense_accuracy_against_float64():
    from _util import record_margin
    case, ref, mag, e32 = _dense()
    dW, db, g_pts, _, _ = _harness().run(*case, prefill=False)
    assert all(np.isfinite(a).all() for a in dW + db) and np.isfinite(g_pts).all()
    e = metric((dW, db), ref, mag)
    print(f"scene flow fused, {DENSE_TILES} tiles: e = {e:.3e}   e_seq32 = {e32:.3e}   e / e_seq32 = {e / e32:.3f}")
    profile_line("RDRF_SF_FUSED_TABLE", f"scene_flow_fused {DENSE_TILES:4d} {e:.3e} {e32:.3e} {e / e32:.3f}")
    record_margin(f"dW scene flow fused ntiles {DENSE_TILES} e / (2 e_seq32)", e / (2.0 * e32))
    assert e <= 2.0 * e32, f"e = {e:.3e} > 2 x e_seq32 = {2.0 * e32:.3e}"


# ---- (c) ------------------------------------------------------------------------------------------------------------------
def _bits(out):
    dW, db, g_pts = out[:3]
    return [a.view(np.uint32) for a in dW + db + [g_pts]]


@pytest.mark.gpu
def test_poison_behind_zero_dz_and_past_the_end():
    H = _harness()
    n = 37 * 32 - 5   # (integer inputs: the sums are exact, so the order of the atomic additions cannot move a bit either)
    rows, W, gf, gb = int_case(n, 21)
    dead = np.random.default_rng(3).random(n) < 0.3
    gf[dead] = 0.0
    gb[dead] = 0.0
    slot_dead = np.ones(rows.shape[0] * 32, dtype=bool)   # the slots past n too
    slot_dead[:n] = dead
    slot_dead = slot_dead.reshape(rows.shape[0], 1, 32)
    benign = np.where(slot_dead, np.float32(1.0), rows)
    hostile = np.where(slot_dead, np.float32(3e38), rows)
    a = H.run(n, benign, W, gf, gb)
    b = H.run(n, hostile, W, gf, gb)
    assert all(np.isfinite(x.view(np.float32)).all() for x in _bits(b))
    assert all(np.array_equal(x, y) for x, y in zip(_bits(a), _bits(b))), "3e38 behind a zero dz or past N * S changed a bit"
    assert any(np.abs(w).max() > 0 for w in b[0])


@pytest.mark.gpu
def test_workspace_contents_do_not_matter():
    H = _harness()
    n = 5 * 32 + 7
    rows, W, gf, gb = int_case(n, 9)
    a = H.run(n, rows, W, gf, gb, ws_byte=0)
    b = H.run(n, rows, W, gf, gb, ws_byte=0xFF)
    assert all(np.array_equal(x, y) for x, y in zip(_bits(a), _bits(b)))


# ---- (d) the tools build: fused against the two-kernel path ----------------------------------------------------------------
def ab_case():
    """what both settings of RDRF_SF_FUSED compute (tests/_det_child.py case)"""
    H = Harness()
    res = {}
    for n in exact_counts():
        dW, db, g_pts = check_exact(H.run, n, 0)
        for i in range(4):
            res[f"x{n}.w{i}"], res[f"x{n}.b{i}"] = dW[i], db[i]
        res[f"x{n}.pts"] = g_pts
    n, rows, W, gf, gb = dense_case(0)
    dW, db, g_pts, _, _ = H.run(n, rows, W, gf, gb, prefill=False)
    for i in range(4):
        res[f"d.w{i}"], res[f"d.b{i}"] = dW[i], db[i]
    res["d.pts"] = g_pts
    return res


@pytest.mark.gpu
def test_fused_against_two_kernel_path(tmp_path):
    got = {}
    for fused in ("1", "0"):
        res = run_twin(tmp_path, [CHILD, "case", "test_gpu_scene_flow_fused", "ab_case"], lib=tools_lib(), extra_env={"RDRF_SF_FUSED": fused})
        got[fused] = {k: v.numpy() for k, v in res.items()}
    assert sorted(got["1"]) == sorted(got["0"])
    for k in sorted(got["1"]):
        a, b = got["1"][k], got["0"][k]
        if k.startswith("x") or k.endswith(".pts"):
            assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{k}: the two paths differ in their bits"
    _, ref, mag, e32 = _dense()
    for fused in ("1", "0"):
        e = metric(([got[fused][f"d.w{i}"] for i in range(4)], [got[fused][f"d.b{i}"] for i in range(4)]), ref, mag)
        print(f"tools build, RDRF_SF_FUSED={fused}: e = {e:.3e}   e_seq32 = {e32:.3e}")
        assert e <= 2.0 * e32, (fused, e, e32)

