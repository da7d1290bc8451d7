"""The heads' backward tile of the dynamic field's density phase and the time branch, each alone on rows and arrays the test
supplies, against the float64 references and the derived bounds of tests/_heads_prim.py (its docstring has the derivations; no
tolerance here was set from a measurement):
  rdrf_selftest_heads_bwd        k_dyn_density_bwd<0, false, true> on flat tiles, k_dyn_density_bwd<0, true> in feature mode
  rdrf_selftest_time_branch      k_time_branch (time_branch_body)
  rdrf_selftest_time_branch_bwd  k_time_branch_bwd with dtout_of_ray
through the launchers and the launch geometry of the entry points.

Heads: every gradient row is pre-filled with a NaN pattern, so a row the kernel must not write (a dead head's dz and d(feature)
rows, the small-layer rows 0..2, everything outside its rows) is compared bit for bit with the pre-fill and a row it must write
cannot pass by accident.  The saved rows hold NaN wherever the kernel must not read and 3e38 in the lanes past the last sample;
the gate values +0.0, -0.0, 2^-126 and ordinary values of both signs sit next to each other in every saved H row (denormals are
left out: whether a denormal input of the comparison is flushed is not part of the contract).  An output whose reference is
exactly 0 (invalid samples, closed gates, padding lanes, padding rows) has the bound 0 and must be exactly 0.
Time branch backward: every dtout / dtp slot dtout_of_ray must not read holds NaN, so a misread shows as a non-finite gradient;
the relu gate classes of the generator (exactly 0 by construction, or 16 forward bounds away) leave nothing to exclude.
Every comparison records error / bound with record_margin (profiles/heads_time_margins.txt holds one run)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _heads_prim as Q   # noqa: E402
from _util import pkg, record_margin   # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 256
NANBITS = 0xFFFFFFFF
REPLACED = ("l1w", "l1b", "l2w", "l2b", "dw1", "db1", "dw2", "db2", "bw1", "bb1", "bw2", "bb2")
ACT = {"relu": 0, "softplus": 1}
SMALL = ("dw2", "db2", "bw2", "bb2")
TIME = ("l1w", "l1b", "l2w", "l2b")


def _pidx():
    """position of each replaced tensor in the dynamic field's parameter list, from the field names of RdrfDynamicParams: the list
    is the planes and lines of the factor sets (six tensors per RdrfVM field), then one tensor per pointer field in struct order
    (robust-dynrf_amd/_params.py _dynamic_struct)"""
    L = pkg()
    fields = L.RdrfDynamicParams._fields_
    nvm = sum(1 for _, t in fields if t is L.RdrfVM)
    names = [n for n, t in fields if t is not L.RdrfVM]
    return {k: 6 * nvm + names.index(k) for k in REPLACED}


PIDX = _pidx()


class Guarded:
    """a device array between two guard bands of the NaN pattern"""

    def __init__(self, host):
        host = np.ascontiguousarray(host)
        self.shape, n = host.shape, host.size
        self.flat = torch.from_numpy(np.full(n + 2 * GUARD, Q.NAN, dtype=np.float32)).cuda()
        self.t = self.flat[GUARD:GUARD + n]
        self.t.copy_(torch.from_numpy(host.reshape(-1)))

    def guards_intact(self):
        g = torch.cat([self.flat[:GUARD], self.flat[-GUARD:]]).cpu().numpy().view(np.uint32)
        return bool((g == NANBITS).all())

    def host(self):
        return self.t.cpu().numpy().reshape(self.shape)


class Harness:
    """a small dynamic field for the parameter struct (the backward packs every weight of the field), its weights replaced per call"""

    def __init__(self):
        import rodynrf
        from _gpu_util import COMMON
        self.L = pkg()
        self.F = pkg("fields")
        aabb = torch.tensor([[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]])
        kw = dict(COMMON, near_far=[0.0, 1.0], density_shift=Q.SHIFT, fea2denseAct="relu")
        torch.manual_seed(3)
        self.dy = rodynrf.TensorVMSplit_TimeEmbedding(aabb, [24, 26, 16], 12, "cuda:0", shadingMode="MLP_Fea_late_view", fea_pe=0, **kw)
        self.params = [p.detach() for p in self.dy._param_list()]
        for k, i in PIDX.items():
            want = {"l1w": (64, 17), "l1b": (64,), "l2w": (30, 64), "l2b": (30,), "dw1": (64, 152), "db1": (64,), "dw2": (1, 64), "db2": (1,),
                    "bw1": (64, 152), "bb1": (64,), "bw2": (1, 64), "bb2": (1,)}[k]
            assert tuple(self.params[i].shape) == want, (k, tuple(self.params[i].shape))
        named = dict(self.dy.named_parameters())   # and by name: the biases of one length cannot be told apart by shape
        for k, name in (("l1w", "layer1.weight"), ("l1b", "layer1.bias"), ("l2b", "layer2.bias"), ("dw1", "density_layer1.weight"),
                        ("db1", "density_layer1.bias"), ("db2", "density_layer2.bias"), ("bw2", "blending_layer2.weight"),
                        ("bb1", "blending_layer1.bias"), ("bb2", "blending_layer2.bias")):
            assert self.params[PIDX[k]].data_ptr() == named[name].data_ptr(), (k, name)
        self.lay = Q.layout(self.L)
        self.ws = torch.zeros(self.L.lib.rdrf_selftest_heads_bwd_workspace_bytes(1, 1), dtype=torch.uint8, device="cuda:0")

    def structs(self, W, pre, names):
        """-> P with the weights W, G whose gradient pointers `names` are Guarded copies of pre; the keep-alive list"""
        params, grads, keep, gb = list(self.params), list(self.params), [], {}
        for k, v in W.items():
            params[PIDX[k]] = torch.from_numpy(np.ascontiguousarray(v)).cuda()
        for k in names:
            gb[k] = Guarded(pre[k])
            grads[PIDX[k]] = gb[k].t
        keep += params + grads
        return self.F._dynamic_struct(params), self.F._dynamic_struct(grads), gb, keep

    def heads(self, c, W, pre, with_dfs=False):
        """-> grows [T][rows][32] (numpy), dfs [n][rec] or None, {name: gradient after the call}"""
        L, lay = self.L, self.lay
        n, T = c["n"], (c["n"] + 31) // 32
        feat = c["mode"] == "feat"
        P, G, gb, keep = self.structs(W, pre, SMALL)
        cfg = self.F._cfg_struct(self.dy, "ndc")
        cfg.act, cfg.density_shift = ACT[c["act"]], c["shift"]
        act = torch.from_numpy(Q.heads_rows(c, lay)).cuda()
        grw = Guarded(np.full((T, lay["grows"], 32), Q.NAN, dtype=np.float32))
        dfs = Guarded(np.full((n, lay["rec"]), Q.NAN, dtype=np.float32)) if with_dfs else None
        dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
        raw, valid = dev(c["raw"]), dev(c["valid"])
        gs, gbl = dev(c["g_sigma"] if feat else c["gsig"]), dev(c["g_b"])
        L.check(L.lib.rdrf_selftest_heads_bwd(C.byref(P), C.byref(cfg), 1 if feat else 0, c["N"], c["S"], L.ptr(act), C.c_size_t(act.numel()),
                                              L.ptr(raw), L.ptr(valid), L.ptr(gs), L.ptr(gbl), int(c["live_d"]), L.ptr(grw.t),
                                              C.c_size_t(grw.t.numel()), L.ptr(dfs.t if with_dfs else None),
                                              C.c_size_t(dfs.t.numel() if with_dfs else 0), C.byref(G), L.ptr(self.ws),
                                              C.c_size_t(self.ws.numel()), L.stream_of(act)), "rdrf_selftest_heads_bwd")
        torch.cuda.synchronize()
        for g, name in [(grw, "grows1"), (dfs, "dfs")] + [(gb[k], k) for k in SMALL]:
            assert g is None or g.guards_intact(), f"the guard bands of {name} were written"
        del keep
        return grw.host(), (dfs.host() if with_dfs else None), {k: gb[k].host() for k in SMALL}


_H = []


def _harness():
    if not _H:
        _H.append(Harness())
    return _H[0]


def _prefill(seed=7):
    rng = np.random.default_rng(seed)
    return {"dw2": rng.standard_normal((1, 64), dtype=np.float32), "db2": rng.standard_normal(1, dtype=np.float32),
            "bw2": rng.standard_normal((1, 64), dtype=np.float32), "bb2": rng.standard_normal(1, dtype=np.float32)}


def _check_heads(H, c, W, tag):
    """one call without records: every row against the reference, the pre-fill or zero; -> the gradient rows"""
    lay, n = H.lay, c["n"]
    T = (n + 31) // 32
    pre = _prefill()
    geo = Q.heads_describe(H.L, 1 if c["mode"] == "feat" else 0, c["N"], c["S"])
    assert geo["tiles"] == T
    ref = Q.heads_reference(c, lay, W, geo, pre)
    grw, _, grads = H.heads(c, W, pre)
    bits = grw.view(np.uint32)
    written = np.zeros(lay["grows"], dtype=bool)
    written[lay["DX0"]:lay["DX0"] + 64] = True
    written[[lay["SM"][0], lay["SM"][1]]] = True
    live = (c["live_d"], c["live_b"])
    for head in range(2):
        for row0, cnt in ((lay["DZ"][head], 64), (lay["DF"][head], 96)):
            if live[head]:
                written[row0:row0 + cnt] = True
            else:
                assert (bits[:, row0:row0 + cnt] == NANBITS).all(), f"{tag}: rows of the dead head {head} were written"
    assert (bits[:, ~written] == NANBITS).all(), f"{tag}: a row outside the heads' rows was written"
    assert (bits[:, lay["SM"][0] - 3:lay["SM"][0]] == NANBITS).all(), f"{tag}: small-layer rows 0..2 were written"
    assert np.isfinite(grw[:, written]).all(), f"{tag}: a written row holds a non-finite value"
    if n % 32:
        assert (grw[-1][written][:, n % 32:] == 0).all(), f"{tag}: a padding lane of a written row is not 0"
    got = {"sm": np.stack([Q.rows_of(grw, lay["SM"][h], 1, n)[:, 0] for h in range(2)], -1), "dX0": Q.rows_of(grw, lay["DX0"], 64, n)}
    worst = {k: Q.ratio(got[k], *ref[k]) for k in got}
    invalid = c["valid"] == 0 if c["mode"] == "flat" else np.zeros(n, dtype=bool)
    assert (got["sm"][invalid] == 0).all() and (got["dX0"][invalid] == 0).all(), f"{tag}: an invalid sample's rows are not 0"
    assert (got["dX0"][:, lay["xcols"] < 0] == 0).all()
    for head in range(2):
        if not live[head]:
            continue
        dz, dF = Q.rows_of(grw, lay["DZ"][head], 64, n), Q.rows_of(grw, lay["DF"][head], 96, n)
        assert (dz[invalid] == 0).all() and (dF[invalid] == 0).all() and (dF[:, lay["fcols"] < 0] == 0).all()
        assert (dz[~(c["H"][head] > 0)] == 0).all(), f"{tag}: a closed gate let a gradient through"
        worst[f"dz{head}"] = Q.ratio(dz, ref["dz"][0][head], ref["dz"][1][head])
        worst[f"dF{head}"] = Q.ratio(dF, ref["dF"][0][head], ref["dF"][1][head])
    for k in SMALL:
        if c["mode"] == "feat" or not live[0 if k[0] == "d" else 1]:
            assert np.array_equal(grads[k].view(np.uint32), pre[k].view(np.uint32)), f"{tag}: {k} was touched"
        else:
            worst[k] = Q.ratio(grads[k].reshape(-1), *ref[k])
    for k, r in worst.items():
        print(f"{tag} {k}: error / bound = {r:.4f}")
        record_margin(f"{tag} {k}", r)
    assert all(r <= 1.0 for r in worst.values()), (tag, worst)
    return grw


@pytest.mark.parametrize("act", ["relu", "softplus"])
@pytest.mark.parametrize("N,S", Q.FLAT_SHAPES)
def test_heads_flat_tiles(N, S, act):
    H, W = _harness(), Q.heads_weights()
    lay = H.lay
    for live in Q.LIVE_SETS:
        c = Q.heads_case("flat", N, S, act, live)
        tag = f"heads flat {N}x{S} {act} live {''.join(live)}"
        rows = _check_heads(H, c, W, tag)
        # records against rows: the same bits through the reported layout, and the d(feature) rows keep their pre-fill
        grw, dfs, _ = H.heads(c, W, _prefill(), with_dfs=True)
        for head, on in enumerate((c["live_d"], c["live_b"])):
            rec = dfs[:, head * lay["set_floats"]:(head + 1) * lay["set_floats"]].view(np.uint32)
            assert (grw.view(np.uint32)[:, lay["DF"][head]:lay["DF"][head] + 96] == NANBITS).all(), f"{tag}: d(feature) rows written beside the records"
            if not on:
                assert (rec == NANBITS).all(), f"{tag}: records of the dead head {head} were written"
                continue
            want = Q.rows_of(rows, lay["DF"][head], 96, c["n"]).view(np.uint32)
            for row, _, _, _, slot in lay["fmap"]:
                assert np.array_equal(rec[:, slot], want[:, row]), f"{tag}: record slot {slot} differs from row {row}"
        other = np.ones(lay["grows"], dtype=bool)
        for head in range(2):
            other[lay["DF"][head]:lay["DF"][head] + 96] = False
        assert np.array_equal(grw.view(np.uint32)[:, other], rows.view(np.uint32)[:, other]), f"{tag}: the records changed another row"


@pytest.mark.parametrize("M", Q.FEAT_SIZES)
def test_heads_feature_mode(M):
    H, W = _harness(), Q.heads_weights(1)
    for live in Q.LIVE_SETS:
        _check_heads(H, Q.heads_case("feat", M, 1, "relu", live), W, f"heads feat {M} live {''.join(live)}")


@pytest.mark.parametrize("N,S", [Q.FLAT_WAVES, Q.FLAT_WALK])
def test_heads_flat_across_waves_and_tiles(N, S):
    """more than 256 tiles: two waves per workgroup (the LDS sum over the waves has two terms); more than 2048: waves walk a second
    tile (running sums, the persistent stride) -- tests/test_heads_primitives_cpu.py asserts both geometries"""
    H = _harness()
    geo = Q.heads_describe(H.L, 0, N, S)
    assert geo["waves"] > 1 and ((N, S) != Q.FLAT_WALK or geo["tiles"] > geo["grid"] * geo["waves"])
    _check_heads(H, Q.heads_case("flat", N, S, "softplus", ("d", "b")), Q.heads_weights(), f"heads flat {N}x{S} softplus live db")


@pytest.mark.parametrize("N,S", [(35, 33), Q.FLAT_WAVES, Q.FLAT_WALK])
def test_heads_small_layer_sums_are_exact_on_integers(N, S):
    H, W = _harness(), Q.heads_weights()
    W = dict(W, dw2=np.rint(4 * W["dw2"]).astype(np.float32), bw2=np.rint(4 * W["bw2"]).astype(np.float32))
    c = Q.heads_case("flat", N, S, "relu", ("d", "b"), regime="int")
    g, _ = Q.head_out_grads(c)   # integers: act' = 1 and bl (1 - bl) = 1/4 of a multiple of 4
    pre = {k: np.rint(3 * v) for k, v in _prefill().items()}
    _, _, grads = H.heads(c, W, pre)
    for head, (wn, bn) in enumerate((("dw2", "db2"), ("bw2", "bb2"))):
        want_w = pre[wn].reshape(64).astype(np.float64) + (g[head][:, None] * c["H"][head].astype(np.float64)).sum(0)
        want_b = pre[bn].astype(np.float64) + g[head].sum()
        mag = np.abs(pre[wn].reshape(64)) + (np.abs(g[head])[:, None] * np.abs(c["H"][head].astype(np.float64))).sum(0)
        assert mag.max() < 2 ** 24 and (want_w == np.rint(want_w)).all()   # every partial sum is exact in any order
        assert (np.abs(want_w - pre[wn].reshape(64)) > 0).mean() > 0.9 and mag.min() > 64 * (N * S // 1155)
        assert np.array_equal(grads[wn].reshape(64).astype(np.float64), want_w), f"{wn}: {int((grads[wn].reshape(64) != want_w).sum())} entries differ"
        assert np.array_equal(grads[bn].astype(np.float64), want_b), bn


# ---- time branch ---------------------------------------------------------------------------------------------------------------------
def _tb_weight_sets():
    return [("seeded", Q.tb_weights(0)), ("zero_rows", Q.tb_weights(1, zero_rows=(0, 17, 63)))]


@pytest.mark.parametrize("N", Q.TB_FWD_N)
def test_time_branch_forward(N):
    H = _harness()
    L = H.L
    rng = np.random.default_rng([43, N])
    pool = np.concatenate([np.array(Q.TB_FIXED_T, dtype=np.float32), rng.uniform(-1, 1, 64).astype(np.float32)])
    nfix = len(Q.TB_FIXED_T)   # every fixed time is met at every N: a small N takes them in several calls
    batches = [pool[o:o + N] for o in range(0, nfix, N)] if N < nfix else [pool[:N]]
    for (name, W), t in [(w, b) for w in _tb_weight_sets() for b in batches]:
        P, _, _, keep = H.structs(W, {}, ())
        ts = torch.from_numpy(t).cuda()
        tout = Guarded(np.full((N + 3, 32), Q.NAN, dtype=np.float32))   # three rows past N
        ctr = torch.full((96,), 12345, dtype=torch.int32, device="cuda")
        L.check(L.lib.rdrf_selftest_time_branch(C.byref(P), L.ptr(ts), N, L.ptr(tout.t), L.ptr(ctr), L.stream_of(ts)), "rdrf_selftest_time_branch")
        torch.cuda.synchronize()
        assert tout.guards_intact() and (ctr[:64] == 0).all() and (ctr[64:] == 12345).all()
        got = tout.host()
        assert (got[N:].view(np.uint32) == NANBITS).all(), "rows past N were written"
        fw = Q.tb_forward(W, t)
        assert (got[:N, 30:] == 0).all(), "columns 30 and 31 of tout are stored as 0"
        r = Q.ratio(got[:N], fw["tout"], fw["btout"])
        print(f"time branch fwd N {N} {name}: error / bound = {r:.4f}")
        record_margin(f"time branch fwd N {N} {name}", r)
        assert r <= 1.0, (N, name, r)
        tout2 = Guarded(np.full((N, 32), Q.NAN, dtype=np.float32))
        ctr.fill_(777)
        L.check(L.lib.rdrf_selftest_time_branch(C.byref(P), L.ptr(ts), N, L.ptr(tout2.t), None, L.stream_of(ts)), "rdrf_selftest_time_branch")
        torch.cuda.synchronize()
        assert (ctr == 777).all(), "a null zero64 must leave the counters alone"
        assert np.array_equal(tout2.host().view(np.uint32), got[:N].view(np.uint32)) and tout2.guards_intact()
        del keep


@pytest.mark.parametrize("N", Q.TB_BWD_N)
def test_time_branch_backward(N):
    H = _harness()
    L = H.L
    for name, W in _tb_weight_sets():
        t, _ = Q.tb_times(W, N)
        assert Q.gate_margin(W, t) >= Q.GATE_MARGIN
        rng = np.random.default_rng([47, N])
        pre = {k: rng.standard_normal(W[k].shape, dtype=np.float32) for k in TIME}
        for S, with_dtp in [(S, True) for S in Q.TB_BWD_S] + [(33, False)]:
            dtout, dtp = Q.tb_cotangents(N, S, with_dtp, seed=N)
            ref = Q.tb_backward(W, t, S, dtout, dtp, pre)
            P, G, gb, keep = H.structs(W, pre, TIME)
            ts, d_out = torch.from_numpy(t).cuda(), torch.from_numpy(dtout).cuda()
            d_p = torch.from_numpy(dtp).cuda() if with_dtp else None
            L.check(L.lib.rdrf_selftest_time_branch_bwd(C.byref(P), L.ptr(ts), N, S, L.ptr(d_out), L.ptr(d_p),
                                                        C.c_size_t(d_p.numel() if with_dtp else 0), C.byref(G), L.stream_of(ts)),
                    "rdrf_selftest_time_branch_bwd")
            torch.cuda.synchronize()
            for k in TIME:
                assert gb[k].guards_intact(), k
                got = gb[k].host()
                assert np.isfinite(got).all(), f"N {N} S {S} {name}: {k} is not finite: a slot dtout_of_ray must not read was read"
                r = Q.ratio(got, *ref[k])
                print(f"time branch bwd N {N} S {S} dtp {int(with_dtp)} {name} {k}: error / bound = {r:.4f}")
                record_margin(f"time branch bwd N {N} S {S} dtp {int(with_dtp)} {name} {k}", r)
                assert r <= 1.0, (N, S, with_dtp, name, k, r)
            del keep


def test_error_paths():
    H = _harness()
    L, lay = H.L, H.lay
    W, pre = Q.heads_weights(), _prefill()
    P, G, gb, keep = H.structs(dict(W, **Q.tb_weights()), dict(pre, **{k: np.zeros(s, dtype=np.float32) for k, s in
                                                                        (("l1w", (64, 17)), ("l1b", 64), ("l2w", (30, 64)), ("l2b", 30))}), SMALL + TIME)
    cfg = H.F._cfg_struct(H.dy, "ndc")
    rows = torch.zeros(lay["rows"] * 32, device="cuda")
    grw = torch.zeros(lay["grows"] * 32, device="cuda")
    one = torch.zeros(64, device="cuda")
    v = torch.ones(64, dtype=torch.uint8, device="cuda")
    hb, tb, tbb = L.lib.rdrf_selftest_heads_bwd, L.lib.rdrf_selftest_time_branch, L.lib.rdrf_selftest_time_branch_bwd
    st = L.stream_of(rows)

    def heads(mode=0, N=1, S=1, act=rows, act_n=None, grows_n=None, ws_n=None, dfs=None, dfs_n=0, raw=one):
        return hb(C.byref(P), C.byref(cfg), mode, N, S, L.ptr(act), C.c_size_t(rows.numel() if act_n is None else act_n), L.ptr(raw), L.ptr(v),
                  L.ptr(one), None, 1, L.ptr(grw), C.c_size_t(grw.numel() if grows_n is None else grows_n), L.ptr(dfs), C.c_size_t(dfs_n),
                  C.byref(G), L.ptr(H.ws), C.c_size_t(H.ws.numel() if ws_n is None else ws_n), st)

    assert heads(N=0) == 0 and heads(mode=1, N=0) == 0
    assert heads(mode=2) == -1 and heads(raw=None) == -1 and heads(S=0) == -1 and heads(S=4097) == -1 and heads(act=None) == -1
    assert heads(mode=1, dfs=one, dfs_n=64) == -1
    assert heads(act_n=rows.numel() - 1) == -3 and heads(grows_n=grw.numel() - 1) == -3 and heads(ws_n=H.ws.numel() - 1) == -3
    assert heads(N=2, S=17) == -3 and heads(dfs=one, dfs_n=lay["rec"] - 1) == -3
    assert b"selftest_heads_bwd" in L.lib.rdrf_last_error()
    big = torch.zeros(lay["rows"] * 32 + 4, device="cuda")
    assert heads(act=big[1:], act_n=big.numel() - 1) == -1 and b"aligned" in L.lib.rdrf_last_error()
    cfg.act = 7
    assert heads() == -1 and b"activation" in L.lib.rdrf_last_error()
    cfg.act = 0
    Gs = H.F._dynamic_struct(keep[len(keep) // 2:])
    Gs.bw2 = None
    assert hb(C.byref(P), C.byref(cfg), 0, 1, 1, L.ptr(rows), C.c_size_t(rows.numel()), L.ptr(one), L.ptr(v), L.ptr(one), None, 1, L.ptr(grw),
              C.c_size_t(grw.numel()), None, C.c_size_t(0), C.byref(Gs), L.ptr(H.ws), C.c_size_t(H.ws.numel()), st) == -1
    assert b"small-layer gradient" in L.lib.rdrf_last_error()
    Pn, Gn = H.F._dynamic_struct(keep[:len(keep) // 2]), H.F._dynamic_struct(keep[len(keep) // 2:])
    Pn.l2w, Gn.l1b = None, None
    assert tb(C.byref(Pn), L.ptr(one), 1, L.ptr(one), None, st) == -1 and b"null time-branch weights" in L.lib.rdrf_last_error()
    assert tbb(C.byref(Pn), L.ptr(one), 1, 1, L.ptr(one), None, C.c_size_t(0), C.byref(G), st) == -1
    assert b"null time-branch weights" in L.lib.rdrf_last_error()
    assert tbb(C.byref(P), L.ptr(one), 1, 1, L.ptr(one), None, C.c_size_t(0), C.byref(Gn), st) == -1
    assert b"null time-branch gradient" in L.lib.rdrf_last_error()
    assert tb(C.byref(P), L.ptr(one), 0, L.ptr(one), None, st) == 0 and tb(C.byref(P), None, 1, L.ptr(one), None, st) == -1
    assert tb(None, L.ptr(one), 1, L.ptr(one), None, st) == -1
    assert tbb(C.byref(P), L.ptr(one), 0, 1, L.ptr(one), None, C.c_size_t(0), C.byref(G), st) == 0
    assert tbb(C.byref(P), L.ptr(one), 1, 0, L.ptr(one), None, C.c_size_t(0), C.byref(G), st) == -1
    assert tbb(C.byref(P), L.ptr(one), 1, 1, None, None, C.c_size_t(0), C.byref(G), st) == -1
    assert tbb(C.byref(P), L.ptr(one), 1, 33, L.ptr(one), L.ptr(one), C.c_size_t(127), C.byref(G), st) == -3
    assert b"selftest_time_branch_bwd" in L.lib.rdrf_last_error()
    torch.cuda.synchronize()
    assert all(gb[k].guards_intact() for k in gb)
    del keep
