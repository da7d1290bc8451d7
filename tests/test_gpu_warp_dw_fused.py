"""The warp MLP backward of the flat training path with the weight gradients of layer3 / layer4 formed in the backward-data
kernel (csrc/rdrf_bwd_fused.hip k_dyn_warp_bwd_dw), alone, through rdrf_selftest_warp_bwd on rows the test supplies: act1
[tile][576][32] (X0 | X1 | T | H3 | H4 | ...), grows1 [tile][544][32] (the heads' d(X0) rows are an input), the coordinate
gradients dxw / dxn and g_xyz_prime per sample.  The field's box is [-1, 1]^3, so box.inv = 1 and dd = dxw + g_xyz_prime.

The reference is the layer equations alone, per sample:
    dz4 = [H4 > 0] W5^T dd,  dz3 = [H3 > 0] W4^T dz4,
    dW5 = sum dd (x) H4,  dW4 = sum dz4 (x) H3,  dW3[:, col(e)] = sum dz3 [X0 | T][e],  db_l = sum dz_l,
    d(tout)[ray][e] = sum over the ray's samples of (W3[:, 63 + e]^T dz3),
col(e) being the slot order of layer3's input rows as rdrf_selftest_dw_describe reports it for the density plan.

(1) exact: weights in {-1, 0, 1} with two non-zeros per input column, dxw and g_xyz_prime in {-1, 0, 1}, rows in [-2, 2]: every
    partial sum stays below 2^24 (computed from the case), so no order of accumulation can change a bit: torch.equal with the
    int64 sums, gradients pre-filled with small integers, at N S = 1, 31, 32, 33, 129, 160, 257 and 32 (grid waves + 3) (grid and
    waves from rdrf_selftest_warp_geometry, the helper the launch uses), and with rays of 45 samples (a tile spans rays; d(tout)
    goes through the tiles' partial records).  The data gradients of the same runs -- g_xyz onto its integer pre-fill and the dd
    rows -- are compared bit for bit with the float64 reference of tests/_warp_prim.py (exact on these inputs); g_xyz, dtout and dtp
    sit between NaN guard bands that must stay intact.  Other boxes and dense inputs: tests/test_gpu_warp_primitives.py.
(2) accuracy: dense normal rows at 257 tiles, e = max |dW - dW64| / sum |dz| |in| within 2 x e_seq32, the same metric of an fp32
    evaluation that sums the samples one after the other (the bound tests/test_gpu_dw_primitives.py holds k_dw3 to).
(3) row contract: 3e38 in every activation slot of the samples whose dd is zero and of the slots past N S changes no bit; nor do
    a workspace, the unread saved rows and the unread gradient rows filled with 0xFF bytes against zero-filled ones.
(4) the tools build (RDRF_WARP_FUSED, read once per process: one child per setting): g_xyz, dtout / dtp are bit-identical to
    k_dyn_density_bwd<1, false, true> on every input, the gradients of layers 3, 4, 5 on the exact inputs of (1).  On the dense
    inputs the layer-5 sums are compared at one tile (one wave on both paths: the same order of additions) and held to the bound
    of (2) at 257 tiles: the two kernels walk the tiles with different launch geometries, their per-wave partial sums and the
    order of the atomic additions differ, and neither path repeats its own bits there.  The two-kernel path's e is recorded
    beside the fused kernel's.  The deterministic library gives the same bits twice on the dense rows."""
import ctypes as C

import numpy as np
import pytest
import torch

from _twin import CHILD, run_twin, tools_lib
from _util import pkg, profile_line

ROWS, GROWS = 576, 544
R_X0, R_T, R_H3, R_H4, G_DX0 = 0, 96, 128, 192, 480
SHAPES = {"l3": (64, 93), "l4": (64, 64), "l5": (3, 64)}
PIDX = {"l3": 29, "l4": 31, "l5": 33}   # weight of the layer in the dynamic field's parameter list; its bias follows
LAYERS = ("l3", "l4", "l5")
PREFILL = 3
DENSE_TILES = 257
DT_FILL = 7.0   # dtout / dtp slots the kernel does not write keep this
GUARD = 64      # floats of NaN on either side of g_xyz, dtout and dtp


def _in_cols():
    """row of [X0 (64) | T (32)] -> column of layer3.weight, -1: padding; from the density plan's description"""
    import _dw_prim as P
    desc = P.describe(pkg(), "DENSITY", 0)
    job = [j for j in desc["jobs"] if j["in_dim"] == 93]
    assert len(job) == 1
    cols = np.full(96, -1, dtype=np.int64)
    for row0, c in job[0]["blocks"]:
        at = row0 - R_X0 if row0 < R_T else 64 + row0 - R_T
        cols[at:at + 32] = c
    assert sorted(cols[cols >= 0]) == list(range(93))
    assert list(cols[64:94]) == list(range(63, 93))
    return cols


def geometry(ntiles):
    L = pkg()
    g, w = C.c_int(0), C.c_int(0)
    L.check(L.lib.rdrf_selftest_warp_geometry(int(ntiles), C.byref(g), C.byref(w)), "rdrf_selftest_warp_geometry")
    return g.value, w.value


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def int_case(N, S, seed):
    n = N * S
    rng = np.random.default_rng([13, seed, N, S])
    T = (n + 31) // 32
    act = rng.integers(-2, 3, size=(T, ROWS, 32)).astype(np.float32)
    grw = rng.integers(-2, 3, size=(T, GROWS, 32)).astype(np.float32)
    W = {}
    for k in LAYERS:
        out, inn = SHAPES[k]
        w = np.zeros((out, inn), dtype=np.float32)
        for c in range(inn):
            w[rng.choice(out, size=2, replace=False), c] = rng.choice([-1.0, 1.0], size=2)
        W[k] = w
    dxw = rng.integers(-1, 2, size=(n, 3)).astype(np.float32)
    dxn = rng.integers(-2, 3, size=(n, 3)).astype(np.float32)
    gp = rng.integers(-1, 2, size=(n, 3)).astype(np.float32)
    return dict(N=N, S=S, act=act, grw=grw, W=W, dxw=dxw, dxn=dxn, gp=gp)


def dense_case(seed=0, T=DENSE_TILES, S=41):   # 200 rays of 41 samples: 257 tiles, the last one partly empty
    rng = np.random.default_rng([17, seed, T])
    N = (T * 32 - 5) // S
    n = N * S
    T = (n + 31) // 32
    act = rng.standard_normal((T, ROWS, 32), dtype=np.float32)
    grw = rng.standard_normal((T, GROWS, 32), dtype=np.float32)
    W = {k: rng.standard_normal(SHAPES[k], dtype=np.float32) / np.float32(np.sqrt(SHAPES[k][1])) for k in LAYERS}
    return dict(N=N, S=S, act=act, grw=grw, W=W, dxw=rng.standard_normal((n, 3), dtype=np.float32),
                dxn=rng.standard_normal((n, 3), dtype=np.float32), gp=rng.standard_normal((n, 3), dtype=np.float32))


# ---- reference ------------------------------------------------------------------------------------------------------------
def _chain(c, dtype):
    """[(dz, input)] for layers 3, 4, 5, the input of layer 3 in weight-column order; and dz3"""
    n = c["N"] * c["S"]
    T = c["act"].shape[0]
    a = c["act"].transpose(0, 2, 1).reshape(T * 32, ROWS)[:n].astype(dtype)
    W = {k: v.astype(dtype) for k, v in c["W"].items()}
    dd = (c["dxw"].astype(dtype) + c["gp"].astype(dtype)).astype(dtype)
    H4, H3 = a[:, R_H4:R_H4 + 64], a[:, R_H3:R_H3 + 64]
    XT = np.concatenate([a[:, R_X0:R_X0 + 64], a[:, R_T:R_T + 32]], axis=1)
    dz4 = np.where(H4 > 0, dd @ W["l5"], 0).astype(dtype)
    dz3 = np.where(H3 > 0, dz4 @ W["l4"], 0).astype(dtype)
    cols = _in_cols()
    In3 = np.zeros((n, 93), dtype=dtype)
    In3[:, cols[cols >= 0]] = XT[:, cols >= 0]
    return {"l3": (dz3, In3), "l4": (dz4, H3), "l5": (dd, H4)}


def reference(c, absolute=False):
    """float64 (exact for the integer cases): {layer: dW}, {layer: db}, d(tout) [N][30]"""
    ch = _chain(c, np.float64)
    dz3 = ch["l3"][0]
    dt = (dz3 @ c["W"]["l3"].astype(np.float64)[:, 63:93]).reshape(c["N"], c["S"], 30).sum(axis=1)
    if absolute:
        ch = {k: (np.abs(d), np.abs(i)) for k, (d, i) in ch.items()}
    return {k: d.T @ i for k, (d, i) in ch.items()}, {k: d.sum(axis=0) for k, (d, _) in ch.items()}, dt


def e_seq32(c, ref):
    """error metric of an fp32 evaluation of the same terms, the samples summed one after the other"""
    ch = _chain(c, np.float32)
    mag = reference(c, absolute=True)
    worst = 0.0
    for k, (d, i) in ch.items():
        acc = np.zeros(SHAPES[k], dtype=np.float32)
        bias = np.zeros(SHAPES[k][0], dtype=np.float32)
        tmp = np.empty_like(acc)
        for s in range(d.shape[0]):
            np.multiply(d[s][:, None], i[s][None, :], out=tmp)
            acc += tmp
            bias += d[s]
        worst = max(worst, float((np.abs(acc - ref[0][k]) / mag[0][k]).max()), float((np.abs(bias - ref[1][k]) / mag[1][k]).max()))
    return worst


def metric(out, ref, mag, layers=LAYERS):
    return max(max(float((np.abs(out[q][k].astype(np.float64) - ref[i][k]) / mag[i][k]).max()) for k in layers)
               for i, q in enumerate(("dW", "db")))


def ray_dtout(c, dtout, dtp):
    """d(tout) per ray from the kernel's two outputs, as k_time_branch_bwd sums them (dtout_of_ray, csrc/rdrf_bwd.hip)"""
    N, S = c["N"], c["S"]
    out = np.zeros((N, 32), dtype=np.float64)
    for n in range(N):
        b = n * S
        t0, t1 = b >> 5, (b + S - 1) >> 5
        if t0 == t1:
            out[n] = dtout[n]
        else:
            out[n] = dtp[t0, 0 if (b & 31) == 0 else 1]
            for t in range(t0 + 1, t1 + 1):
                out[n] += dtp[t, 0]
    return out[:, :30]


# ---- the call -------------------------------------------------------------------------------------------------------------
class Harness:
    """a small dynamic field on the box [-1, 1]^3 for the parameter struct (the backward packs every weight of the field)"""

    def __init__(self):
        import rodynrf
        from _gpu_util import COMMON
        self.L = pkg()
        self.F = pkg("fields")
        aabb = torch.tensor([[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]])
        kw = dict(COMMON, near_far=[0.0, 1.0], density_shift=-10.0, fea2denseAct="relu")
        torch.manual_seed(3)
        self.dy = rodynrf.TensorVMSplit_TimeEmbedding(aabb, [24, 26, 16], 12, "cuda:0", shadingMode="MLP_Fea_late_view", fea_pe=0, **kw)
        self.params = [p.detach() for p in self.dy._param_list()]
        self.cfg = self.F._cfg_struct(self.dy, "ndc")

    def cfg_for(self, box):
        """the field's configuration on another box [[lo 3], [hi 3]] (None: the harness's own)"""
        if box is None:
            return self.cfg
        cfg = type(self.cfg).from_buffer_copy(self.cfg)
        for i, v in enumerate(np.asarray(box, dtype=np.float32).reshape(6)):
            cfg.aabb[i] = float(v)
        return cfg

    def run(self, c, gx=True, gp=True, ws_byte=0, prefill=True, det=False, box=None):
        """-> dict of numpy arrays: dW / db per layer, g_xyz, dtout, dtp, and the pre-fills.  g_xyz (pre-filled with c["pre"] if the
        case has one), dtout and dtp sit between NaN-poisoned guard bands of GUARD floats: "guards" tells whether each pair is intact;
        without gx the kernel gets no g_xyz and "g_xyz_unused" is the buffer it must not have touched"""
        L, dev = self.L, "cuda:0"
        N, S = c["N"], c["S"]
        cfg = self.cfg_for(box)
        n, T = N * S, c["act"].shape[0]
        params = list(self.params)
        rng = np.random.default_rng(5)
        sizes = [int(np.prod(SHAPES[k])) for k in LAYERS] + [SHAPES[k][0] for k in LAYERS]
        pre = (rng.integers(-PREFILL, PREFILL + 1, size=sum(sizes)) if prefill else np.zeros(sum(sizes))).astype(np.float32)
        flat = torch.from_numpy(pre.copy()).to(dev)   # (one buffer: the deterministic library binds it to its shadow)
        views, o = [], 0
        for sz in sizes:
            views.append(flat[o:o + sz])
            o += sz
        grads = list(self.params)
        for i, k in enumerate(LAYERS):
            params[PIDX[k]] = torch.from_numpy(c["W"][k]).to(dev).contiguous()
            params[PIDX[k] + 1] = torch.zeros(SHAPES[k][0], device=dev)
            grads[PIDX[k]], grads[PIDX[k] + 1] = views[i], views[3 + i]
        P, G = self.F._dynamic_struct(params), self.F._dynamic_struct(grads)
        act = torch.from_numpy(c["act"]).to(dev).contiguous()
        grw = torch.from_numpy(c["grw"]).to(dev).contiguous()
        dxw, dxn = torch.from_numpy(c["dxw"]).to(dev).contiguous(), torch.from_numpy(c["dxn"]).to(dev).contiguous()
        cgp = torch.from_numpy(c["gp"]).to(dev).contiguous() if gp and c["gp"] is not None else None
        pre_g = c["pre"] if c.get("pre") is not None else np.arange(n * 3, dtype=np.float32).reshape(n, 3) % 5
        bands = {k: torch.full((GUARD + m + GUARD,), float("nan"), device=dev) for k, m in (("g_xyz", n * 3), ("dtout", N * 32), ("dtp", T * 64))}
        gbuf = bands["g_xyz"][GUARD:GUARD + n * 3].view(n, 3).copy_(torch.from_numpy(np.ascontiguousarray(pre_g, dtype=np.float32)))
        g_xyz = gbuf if gx else None
        dtout = bands["dtout"][GUARD:GUARD + N * 32].view(N, 32).fill_(DT_FILL)
        dtp = bands["dtp"][GUARD:GUARD + T * 64].view(T, 2, 32).fill_(DT_FILL)
        ws = torch.full((L.lib.rdrf_selftest_warp_bwd_workspace_bytes(N, S),), ws_byte, dtype=torch.uint8, device=dev)
        shadow = None
        if det:
            shadow = torch.zeros(flat.numel(), dtype=torch.int64, device=dev)
            L.check(L.lib.rdrf_det_bind(1, L.ptr(flat), C.c_size_t(flat.numel()), L.ptr(shadow), L.stream_of(flat)), "rdrf_det_bind")
        L.check(L.lib.rdrf_selftest_warp_bwd(C.byref(P), C.byref(cfg), N, S, L.ptr(act), C.c_size_t(act.numel()), L.ptr(grw),
                                             C.c_size_t(grw.numel()), L.ptr(dxw), L.ptr(dxn), L.ptr(cgp), C.byref(G), L.ptr(g_xyz),
                                             L.ptr(dtout), L.ptr(dtp), L.ptr(ws), C.c_size_t(ws.numel()), L.stream_of(act)),
                "rdrf_selftest_warp_bwd")
        if det:
            L.check(L.lib.rdrf_det_finish(1, L.stream_of(flat)), "rdrf_det_finish")
        torch.cuda.synchronize()
        res = dict(dW={}, db={}, pre_w={}, pre_b={})
        o = 0
        host = flat.cpu().numpy()
        for i, k in enumerate(LAYERS):
            res["dW"][k] = host[o:o + sizes[i]].reshape(SHAPES[k]).copy()
            res["pre_w"][k] = pre[o:o + sizes[i]].reshape(SHAPES[k])
            o += sizes[i]
        for i, k in enumerate(LAYERS):
            res["db"][k] = host[o:o + sizes[3 + i]].copy()
            res["pre_b"][k] = pre[o:o + sizes[3 + i]]
            o += sizes[3 + i]
        res["g_xyz"] = None if g_xyz is None else g_xyz.cpu().numpy()
        res["g_xyz_unused"], res["pre_g"] = (gbuf.cpu().numpy() if g_xyz is None else None), np.asarray(pre_g, dtype=np.float32)
        res["guards"] = {k: bool(torch.isnan(torch.cat([b[:GUARD], b[-GUARD:]])).all()) for k, b in bands.items()}
        res["dtout"], res["dtp"] = dtout.cpu().numpy(), dtp.cpu().numpy()
        res["sm"] = grw[:, 128:131].cpu().numpy()   # the small-layer dz rows 0..2 the kernel writes
        return res


_H = []


def _harness():
    if not _H:
        _H.append(Harness())
    return _H[0]


def exact_cases():
    """(N, S): the counts of the issue with one-sample rays, and rays of 45 samples"""
    grid, waves = geometry(1 << 20)
    big = grid * waves + 3
    assert geometry(big) == (grid, waves)
    return [(n, 1) for n in (1, 31, 32, 33, 129, 160, 257, 32 * big)] + [(3, 45), (23, 45)]


def check_exact(run, N, S, seed, **kw):
    c = int_case(N, S, seed)
    if not kw.get("gp", True):
        c["gp"] = np.zeros_like(c["gp"])
    ref = reference(c)
    mag = reference(c, absolute=True)
    bound = PREFILL + max(float(m[k].max()) for m in mag[:2] for k in LAYERS)
    assert bound < 2 ** 24, bound   # any order of accumulation is exact
    out = run(c, **kw)
    for k in LAYERS:
        want_w = torch.from_numpy(np.rint(ref[0][k]).astype(np.int64) + out["pre_w"][k].astype(np.int64))
        want_b = torch.from_numpy(np.rint(ref[1][k]).astype(np.int64) + out["pre_b"][k].astype(np.int64))
        got_w, got_b = torch.from_numpy(out["dW"][k]), torch.from_numpy(out["db"][k])
        assert torch.equal(got_w.to(torch.int64), want_w) and torch.equal(got_w, want_w.float()), \
            f"N {N} S {S}: dW of {k}: {int((got_w != want_w.float()).sum())} entries differ"
        assert torch.equal(got_b.to(torch.int64), want_b) and torch.equal(got_b, want_b.float()), \
            f"N {N} S {S}: db of {k}: {int((got_b != want_b.float()).sum())} entries differ"
    assert np.array_equal(ray_dtout(c, out["dtout"], out["dtp"]), ref[2]), f"N {N} S {S}: d(tout) differs"
    # the data gradients against the float64 reference of tests/_warp_prim.py: on integers and the unit box every sum is exact
    import _warp_prim as Q
    lay = Q.warp_layout(pkg())
    cq = dict(c, box=Q.BOX_UNIT, pre=out["pre_g"])
    Q.warp_exact_guard(cq, lay)   # asserts that every partial sum stays below 2^24
    want = Q.warp_reference(cq, lay)
    T = c["act"].shape[0]
    assert np.array_equal(out["sm"].transpose(0, 2, 1).reshape(T * 32, 3).astype(np.float64), want["dd"][0]), f"N {N} S {S}: the dd rows differ"
    if out["g_xyz"] is not None:
        assert np.array_equal(out["g_xyz"].astype(np.float64), want["g_xyz"][0]), f"N {N} S {S}: g_xyz differs"
    else:
        assert np.array_equal(out["g_xyz_unused"], out["pre_g"])
    assert all(out["guards"].values()), out["guards"]
    return out


# ---- no GPU: the reference against plain loops ------------------------------------------------------------------------------
def test_reference_against_plain_loops():
    c = int_case(2, 21, 1)
    ref = reference(c)
    cols = _in_cols()
    W = {k: v.astype(np.int64) for k, v in c["W"].items()}
    dW = {k: np.zeros(SHAPES[k], dtype=np.int64) for k in LAYERS}
    db = {k: np.zeros(SHAPES[k][0], dtype=np.int64) for k in LAYERS}
    dt = np.zeros((2, 30), dtype=np.int64)
    for i in range(42):
        t, s = divmod(i, 32)
        col = c["act"][t, :, s].astype(np.int64)
        dd = (c["dxw"][i] + c["gp"][i]).astype(np.int64)
        dz4 = np.array([(W["l5"][:, k] * dd).sum() if col[R_H4 + k] > 0 else 0 for k in range(64)])
        dz3 = np.array([(W["l4"][:, k] * dz4).sum() if col[R_H3 + k] > 0 else 0 for k in range(64)])
        xt = np.concatenate([col[R_X0:R_X0 + 64], col[R_T:R_T + 32]])
        for o in range(64):
            for e in range(96):
                if cols[e] >= 0:
                    dW["l3"][o, cols[e]] += dz3[o] * xt[e]
        dW["l4"] += np.outer(dz4, col[R_H3:R_H3 + 64])
        dW["l5"] += np.outer(dd, col[R_H4:R_H4 + 64])
        db["l3"] += dz3
        db["l4"] += dz4
        db["l5"] += dd
        dt[i // 21] += W["l3"][:, 63:93].T @ dz3
    for k in LAYERS:
        assert np.array_equal(ref[0][k], dW[k].astype(np.float64)) and np.array_equal(ref[1][k], db[k].astype(np.float64))
    assert np.array_equal(ref[2], dt.astype(np.float64)) and np.abs(dt).max() > 0 and np.abs(dW["l3"]).max() > 0


# ---- (1) ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_exact_weight_gradients():
    H = _harness()
    cases = exact_cases()
    for N, S in cases:
        check_exact(H.run, N, S, 0)
    for N, S in cases[:7] + cases[8:]:
        check_exact(H.run, N, S, 1, gx=False)
        check_exact(H.run, N, S, 2, gp=False)


# ---- (2) ------------------------------------------------------------------------------------------------------------------
_DENSE = []


def _dense():
    if not _DENSE:
        c = dense_case()
        ref = reference(c)
        _DENSE.append((c, ref, reference(c, absolute=True), e_seq32(c, ref)))
    return _DENSE[0]


@pytest.mark.gpu
def test_dense_accuracy_against_float64():
    from _util import record_margin
    c, ref, mag, e32 = _dense()
    out = _harness().run(c, prefill=False)
    assert all(np.isfinite(out[q][k]).all() for q in ("dW", "db") for k in LAYERS) and np.isfinite(out["g_xyz"]).all()
    e = metric(out, ref, mag)
    print(f"warp fused, {c['act'].shape[0]} tiles: e = {e:.3e}   e_seq32 = {e32:.3e}   e / e_seq32 = {e / e32:.3f}")
    profile_line("RDRF_WARP_FUSED_TABLE", f"warp_fused     {c['act'].shape[0]:4d} {e:.3e} {e32:.3e} {e / e32:.3f}")
    record_margin(f"dW warp fused ntiles {c['act'].shape[0]} e / (2 e_seq32)", e / (2.0 * e32))
    assert e <= 2.0 * e32, f"e = {e:.3e} > 2 x e_seq32 = {2.0 * e32:.3e}"


# ---- (3) ------------------------------------------------------------------------------------------------------------------
def _bits(out):
    a = [out[q][k] for q in ("dW", "db") for k in LAYERS] + [out["g_xyz"], out["dtout"], out["dtp"], out["sm"]]
    return [x.view(np.uint32) for x in a]


@pytest.mark.gpu
def test_poison_behind_zero_dz_and_past_the_end():
    H = _harness()
    N, S = 26, 45   # 1170 samples: 37 tiles, the last one partly empty
    c = int_case(N, S, 21)
    n = N * S
    dead = np.random.default_rng(3).random(n) < 0.3
    c["dxw"][dead] = 0.0
    c["gp"][dead] = 0.0
    T = c["act"].shape[0]
    slot_dead = np.ones(T * 32, dtype=bool)   # the slots past n too
    slot_dead[:n] = dead
    slot_dead = slot_dead.reshape(T, 1, 32)
    c["grw"][:, G_DX0:G_DX0 + 64] = np.where(slot_dead, np.float32(0.0), c["grw"][:, G_DX0:G_DX0 + 64])   # no upstream: no d(X0)
    rows = c["act"]
    a = H.run(dict(c, act=np.where(slot_dead, np.float32(1.0), rows)))
    b = H.run(dict(c, act=np.where(slot_dead, np.float32(3e38), rows)))
    assert all(np.isfinite(x.view(np.float32)).all() for x in _bits(b))
    assert all(np.array_equal(x, y) for x, y in zip(_bits(a), _bits(b))), "3e38 behind a zero dz or past N * S changed a bit"
    assert all(np.abs(b["dW"][k] - b["pre_w"][k]).max() > 0 for k in LAYERS)


@pytest.mark.gpu
def test_scratch_contents_do_not_matter():
    H = _harness()
    c = int_case(167, 1, 9)
    read_act = np.zeros(ROWS, dtype=bool)
    for r0, nr in ((R_X0, 64), (R_T, 32), (R_H3, 64), (R_H4, 64)):
        read_act[r0:r0 + nr] = True
    read_g = np.zeros(GROWS, dtype=bool)
    read_g[G_DX0:G_DX0 + 64] = True
    nan = np.frombuffer(b"\xff\xff\xff\xff", dtype=np.float32)[0]
    outs = []
    for fill, ws_byte in ((np.float32(0.0), 0), (nan, 0xFF)):
        act = np.where(read_act[None, :, None], c["act"], fill)
        grw = np.where(read_g[None, :, None], c["grw"], fill)
        outs.append(H.run(dict(c, act=act, grw=grw), ws_byte=ws_byte))
    assert all(np.isfinite(x.view(np.float32)).all() for x in _bits(outs[1]))
    assert all(np.array_equal(x, y) for x, y in zip(_bits(outs[0]), _bits(outs[1])))


# ---- (4) the tools build: fused against the two-kernel path; the deterministic library twice --------------------------------
def _flatten(res, out, tag):
    for k in LAYERS:
        res[f"{tag}.w.{k}"], res[f"{tag}.b.{k}"] = out["dW"][k], out["db"][k]
    for k in ("g_xyz", "dtout", "dtp", "sm"):
        res[f"{tag}.{k}"] = out[k]


def ab_case():
    """what both settings of RDRF_WARP_FUSED compute (tests/_det_child.py case)"""
    H = Harness()
    res = {}
    for N, S in exact_cases():
        _flatten(res, check_exact(H.run, N, S, 0), f"x{N}_{S}")
    _flatten(res, H.run(dense_case(), prefill=False), "d")
    _flatten(res, H.run(dense_case(1, T=1, S=9), prefill=False), "o")   # one tile: one wave on both paths
    return res


def det_twice_case():
    """the dense rows twice in the deterministic library"""
    H = Harness()
    res = {}
    c = dense_case()
    for rep in ("r0", "r1"):
        _flatten(res, H.run(c, prefill=False, det=True), rep)
    return res


def _run_child(tmp_path, func, **kw):
    res = run_twin(tmp_path, [CHILD, "case", "test_gpu_warp_dw_fused", func], **kw)
    return {k: v.numpy() for k, v in res.items()}


@pytest.mark.gpu
def test_fused_against_two_kernel_path(tmp_path):
    got = {f: _run_child(tmp_path, "ab_case", lib=tools_lib(), extra_env={"RDRF_WARP_FUSED": f}) for f in ("1", "0")}
    assert sorted(got["1"]) == sorted(got["0"])
    for k in sorted(got["1"]):
        a, b = got["1"][k], got["0"][k]
        data = k.split(".")[1] in ("g_xyz", "dtout", "dtp", "sm")
        if k.startswith("x") or data or (k.startswith("o") and k.endswith("l5")):
            assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{k}: the two paths differ in their bits"
    c, ref, mag, e32 = _dense()
    for f in ("1", "0"):
        out = dict(dW={k: got[f][f"d.w.{k}"] for k in LAYERS}, db={k: got[f][f"d.b.{k}"] for k in LAYERS})
        e = metric(out, ref, mag)
        print(f"tools build, RDRF_WARP_FUSED={f}: e = {e:.3e}   e_seq32 = {e32:.3e}")
        profile_line("RDRF_WARP_FUSED_TABLE", f"tools_fused={f}  {c['act'].shape[0]:4d} {e:.3e} {e32:.3e} {e / e32:.3f}")
        assert e <= 2.0 * e32, (f, e, e32)


@pytest.mark.gpu
def test_deterministic_library_repeats_its_bits(tmp_path):
    got = _run_child(tmp_path, "det_twice_case", det=True)
    keys = sorted(k[3:] for k in got if k.startswith("r0."))
    assert keys and all(np.array_equal(got["r0." + k].view(np.uint32), got["r1." + k].view(np.uint32)) for k in keys)
    c, ref, mag, e32 = _dense()
    out = dict(dW={k: got[f"r0.w.{k}"] for k in LAYERS}, db={k: got[f"r0.b.{k}"] for k in LAYERS})
    assert metric(out, ref, mag) <= 2.0 * e32

