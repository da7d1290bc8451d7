"""No GPU: keeps tests/_heads_prim.py honest (the references, generators and bounds of test_gpu_heads_primitives.py).
  * each reference equals torch autograd in float64 over the same subgraph, built from oracle/rodynrf_oracle.py pieces;
  * a plain float32 evaluation of the same operation meets every bound;
  * the generators' conditions hold: the relu gate margin of the time branch (no case is excluded: the share is zero), the gate
    values, activation edges and invalid samples of the heads' cases land where intended, the NaN slots of the cotangents are
    exactly the ones dtout_of_ray must not read;
  * the reference of dtout_of_ray equals a brute-force per-sample sum at every (N, S) used;
  * the layouts the library reports are consistent with each other, and the three entry points are declared."""
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _util import pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _heads_prim as Q   # noqa: E402
from oracle import rodynrf_oracle as O   # noqa: E402

NEW = ("rdrf_selftest_heads_bwd_workspace_bytes", "rdrf_selftest_heads_describe", "rdrf_selftest_heads_bwd", "rdrf_selftest_time_branch",
       "rdrf_selftest_time_branch_bwd")
_LAY = []


def _lay():
    if not _LAY:
        _LAY.append(Q.layout(pkg()))
    return _LAY[0]


def test_entry_points_are_declared():
    L = pkg()
    header = open(os.path.join(ROOT, "include", "rodynrf.h")).read()
    for name in NEW:
        assert name in L.SIGNATURES and hasattr(L.lib, name) and re.search(r"\b%s\(" % name, header), name
    assert L.lib.rdrf_selftest_heads_bwd_workspace_bytes(1, 1) == 4 * L.lib.rdrf_pack_floats()


def test_layouts_agree_with_each_other():
    lay = _lay()
    assert sorted(np.concatenate(lay["H"]).tolist()) == sorted(set(np.concatenate(lay["H"]).tolist())) and lay["SM"][1] == lay["SM"][0] + 1
    # a d(feature) row's first-layer column is its logical [level][plane][component] index: 16 + 4 + 4 components per level
    for row, lv, plane, comp, slot in lay["fmap"]:
        assert lay["fcols"][row] == 24 * lv + (0, 16, 20)[plane] + comp and 0 <= slot < lay["set_floats"]
    assert sorted(s for *_, s in lay["fmap"]) == list(range(lay["nfeat"])) and 2 * lay["set_floats"] == lay["rec"]
    spans = sorted([(lay["DZ"][0], 64), (lay["DZ"][1], 64), (lay["DF"][0], 96), (lay["DF"][1], 96), (lay["DX0"], 64), (lay["SM"][0] - 3, 5)])
    assert all(a + n <= b for (a, n), (b, _) in zip(spans, spans[1:])) and spans[-1][0] + spans[-1][1] <= lay["grows"]
    L = pkg()
    for N, S in Q.FLAT_SHAPES:
        g = Q.heads_describe(L, 0, N, S)
        assert g["tiles"] == (N * S + 31) // 32 and g["grid"] * g["waves"] >= min(g["tiles"], 256) and 1 <= g["waves"] <= 8
    assert [Q.heads_describe(L, 1, M)["tiles"] for M in Q.FEAT_SIZES] == [(M + 31) // 32 for M in Q.FEAT_SIZES]


# ---- heads -------------------------------------------------------------------------------------------------------------------------
def _autograd_heads(c, W, lay):
    """the two heads from their first layer on, in float64: x [n][152] -> H = relu(W1 x) -> raw = w2 H -> sigma, blending; the
    case's H and raw are this graph's own values, so the reference sees what autograd sees"""
    n = c["n"]
    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.standard_normal((n, 152))).requires_grad_(True)
    sd = {}
    for p in ("density", "blending"):
        sd[p + "_layer1.weight"] = torch.from_numpy(W[p[0] + "w1"].astype(np.float64))
        sd[p + "_layer1.bias"] = torch.from_numpy(rng.standard_normal(64) * 0.1)
        sd[p + "_layer2.weight"] = torch.from_numpy(W[p[0] + "w2"].astype(np.float64)).requires_grad_(True)
        sd[p + "_layer2.bias"] = torch.zeros(1, dtype=torch.float64, requires_grad=True)
    Hs = [F.relu(O._lin(x, sd, p + "_layer1")) for p in ("density", "blending")]
    raws = [O._lin(H, sd, p + "_layer2")[..., 0] for H, p in zip(Hs, ("density", "blending"))]
    c = dict(c, H=np.stack([H.detach().numpy() for H in Hs]), raw=np.stack([r.detach().numpy() for r in raws], -1))
    valid = torch.from_numpy(c["valid"] != 0)
    loss = x.sum() * 0.0
    if c["mode"] == "flat":
        sigma = F.softplus(raws[0] + c["shift"], threshold=1e9) if c["act"] == "softplus" else O.feature2density(raws[0], "relu", c["shift"])
        if c["live_d"]:
            loss = loss + (torch.from_numpy(c["gsig"].astype(np.float64)) * sigma)[valid].sum()
        if c["live_b"]:
            loss = loss + (torch.from_numpy(c["g_b"].astype(np.float64)) * torch.sigmoid(raws[1]))[valid].sum()
    else:
        for key, r in (("g_sigma", raws[0]), ("g_b", raws[1])):
            if c[key] is not None:
                loss = loss + (torch.from_numpy(c[key].astype(np.float64)) * r).sum()
    leaves = [x] + [sd[p + "_layer2." + q] for p in ("density", "blending") for q in ("weight", "bias")]
    grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    return c, [None if g is None else g.numpy() for g in grads]


@pytest.mark.parametrize("mode,act,live", [("flat", "relu", ("d", "b")), ("flat", "softplus", ("d", "b")), ("flat", "softplus", ("d",)),
                                           ("flat", "relu", ("b",)), ("feat", "relu", ("d", "b")), ("feat", "relu", ("b",))])
def test_heads_reference_equals_autograd(mode, act, live):
    lay, W = _lay(), Q.heads_weights()
    c = Q.heads_case(mode, 5, 13, act, live, seed=1)
    c["shift"] = 0.5   # (the graph's own raw outputs are of order 0.1: keep the sigmoid away from its tail)
    c, (gx, dw2, db2, bw2, bb2) = _autograd_heads(c, W, lay)
    # one total d(features) per column: autograd adds the two heads, so each head is taken alone where both are live
    geo = dict(tiles=3, grid=3, waves=1)
    pre = {k: np.zeros(64 if k[1] == "w" else 1) for k in ("dw2", "db2", "bw2", "bb2")}
    ref = Q.heads_reference(c, lay, W, geo, pre)
    fc, xc = lay["fcols"], lay["xcols"]
    want_F = sum(ref["dF"][0][h] for h in range(2))
    assert np.abs(want_F[:, fc >= 0] - gx[:, fc[fc >= 0]]).max() < 1e-12 and (want_F[:, fc < 0] == 0).all()
    assert np.abs(ref["dX0"][0][:, xc >= 0] - gx[:, xc[xc >= 0]]).max() < 1e-12 and (ref["dX0"][0][:, xc < 0] == 0).all()
    assert np.abs(gx).max() > 1e-3
    if mode == "flat":
        for name, g in (("dw2", dw2), ("db2", db2), ("bw2", bw2), ("bb2", bb2)):
            g = np.zeros_like(ref[name][0]) if g is None else g.reshape(-1)   # a dead head: autograd never visits it
            assert np.abs(ref[name][0] - g).max() < 1e-12, name
        assert "d" not in live or np.abs(dw2).max() > 0


@pytest.mark.parametrize("mode,shape", [("flat", s) for s in Q.FLAT_SHAPES] + [("feat", (m, 1)) for m in Q.FEAT_SIZES])
@pytest.mark.parametrize("act", ["relu", "softplus"])
def test_heads_float32_evaluation_meets_every_bound(mode, shape, act):
    lay, W, L = _lay(), Q.heads_weights(), pkg()
    c = Q.heads_case(mode, shape[0], shape[1], act, ("d", "b"), seed=2)
    geo = Q.heads_describe(L, 0 if mode == "flat" else 1, shape[0], shape[1])
    pre = {k: np.zeros(64 if k[1] == "w" else 1) for k in ("dw2", "db2", "bw2", "bb2")}
    ref, got = Q.heads_reference(c, lay, W, geo, pre), Q.heads_eval32(c, lay, W, geo, pre)
    names = ("sm", "dz", "dF", "dX0") + (("dw2", "db2", "bw2", "bb2") if mode == "flat" else ())
    for name in names:
        r = Q.ratio(got[name], *ref[name])
        assert r <= 1.0, (name, r)
        assert np.isfinite(ref[name][1]).all()


def test_heads_small_sums_across_waves_and_tiles():
    """the two large shapes of the GPU file: more than one wave per workgroup, and waves that walk more than one tile; the small-layer
    sums of a float32 evaluation in the kernel's order meet the derived bound there as well"""
    L = pkg()
    g = Q.heads_describe(L, 0, *Q.FLAT_WAVES)
    assert g["waves"] > 1 and g["grid"] > 1 and g["grid"] * g["waves"] >= g["tiles"]
    gw = Q.heads_describe(L, 0, *Q.FLAT_WALK)
    assert gw["waves"] > 1 and gw["tiles"] > gw["grid"] * gw["waves"], gw   # tiles per wave > 1
    c = Q.heads_case("flat", *Q.FLAT_WAVES, "relu", ("d", "b"), seed=3)
    rng = np.random.default_rng(9)
    pre = {k: rng.standard_normal(64 if k[1] == "w" else 1).astype(np.float32) for k in ("dw2", "db2", "bw2", "bb2")}
    gr, bg = Q.head_out_grads(c)
    g32 = Q.heads_eval32(c, _lay(), Q.heads_weights())["sm"].T
    for geo in (g, dict(gw, tiles=g["tiles"], grid=16, waves=8)):   # (the second: the case's 266 tiles on 128 waves, three tiles each)
        tpw = -(-geo["tiles"] // (geo["grid"] * geo["waves"]))
        assert tpw > 1 or geo is g
        for head, (wn, bn) in enumerate((("dw2", "db2"), ("bw2", "bb2"))):
            H64 = c["H"][head].astype(np.float64)
            terms = gr[head][:, None] * H64
            kw, kb = 1 + 5 + tpw + geo["waves"] + geo["grid"], tpw + 6 + geo["waves"] + geo["grid"]
            bw = (bg[head][:, None] * np.abs(H64)).sum(0) + kw * Q.U * (np.abs(pre[wn]) + np.abs(terms).sum(0)) + Q.TINY * (terms != 0).sum(0)
            bb = bg[head].sum() + kb * Q.U * (np.abs(pre[bn]) + np.abs(gr[head]).sum())
            sw, sb = Q.small_sums32(g32[head], c["H"][head], geo, pre[wn], pre[bn])
            assert Q.ratio(sw, pre[wn].astype(np.float64) + terms.sum(0), bw) <= 1.0 and Q.ratio(sb, pre[bn].astype(np.float64) + gr[head].sum(), bb) <= 1.0


def test_heads_generator_conditions():
    lay = _lay()
    for act in ("relu", "softplus"):
        c = Q.heads_case("flat", 35, 33, act, ("d", "b"))
        H = c["H"]
        bits = H.view(np.uint32)
        for pattern in (0x00000000, 0x80000000, 0x00800000):   # +0.0, -0.0, 2^-126
            assert (bits == pattern).mean() > 0.1
        assert (H > 1e-6).mean() > 0.2 and (H < -1e-6).mean() > 0.1
        assert not ((bits & 0x7f800000 == 0) & (bits & 0x007fffff != 0)).any(), "denormals are left out"
        # next to each other: every sample's row holds every kind
        assert all(((bits[h] == 0).any(-1) & (bits[h] == 0x80000000).any(-1) & (bits[h] == 0x00800000).any(-1)).all() for h in range(2))
        x = c["raw"][:, 0].astype(np.float64) + (c["shift"] if act == "softplus" else 0.0)
        edges = Q.LOGITS if act == "softplus" else Q.RELU_FD
        assert all(((x == v) & (c["valid"] != 0)).any() for v in edges), act
        assert all(((c["raw"][:, 1] == v) & (c["valid"] != 0)).any() for v in Q.LOGITS)
        assert 0.05 < (c["valid"] == 0).mean() < 0.4
        rows = Q.heads_rows(c, lay)
        assert np.array_equal(Q.rows_of(rows, 0, lay["rows"], c["n"])[:, lay["H"][1]], c["H"][1])
        assert np.isnan(rows).mean() > 0.7 and (rows[-1, lay["H"][0], c["n"] % 32:] == np.float32(3e38)).all()
    c = Q.heads_case("flat", 3, 11, "relu", ("d",))
    assert c["valid"][32] == 1 and c["g_b"] is None
    ci = Q.heads_case("flat", 35, 33, "relu", ("d", "b"), regime="int")
    g, b = Q.head_out_grads(ci)
    assert (g == np.rint(g)).all() and np.abs(g).max() > 0 and np.abs(g[1]).max() <= 3


# ---- time branch -------------------------------------------------------------------------------------------------------------------
def _sd(W, requires_grad=False):
    m = {"l1w": "layer1.weight", "l1b": "layer1.bias", "l2w": "layer2.weight", "l2b": "layer2.bias"}
    return {m[k]: torch.from_numpy(v.astype(np.float64)).requires_grad_(requires_grad) for k, v in W.items()}


def test_time_branch_reference_equals_the_oracle_and_autograd():
    W = Q.tb_weights(0, zero_rows=(3, 40))
    N, S = 33, 33
    t, _ = Q.tb_times(W, N)
    sd = _sd(W, True)
    out = O.time_branch(sd, torch.from_numpy(t.astype(np.float64)))
    fw = Q.tb_forward(W, t)
    assert np.abs(fw["tout"][:, :30] - out.detach().numpy()).max() < 1e-12 and (fw["tout"][:, 30:] == 0).all()
    dtout, dtp = Q.tb_cotangents(N, S, True)
    dz2, _, cnt = Q.dtout_of_ray(dtout, dtp, N, S)
    assert cnt.max() >= 2 and np.isfinite(dz2).all()
    pre = {k: np.zeros(v.shape) for k, v in W.items()}
    ref = Q.tb_backward(W, t, S, dtout, dtp, pre)
    grads = torch.autograd.grad((out * torch.from_numpy(dz2)).sum(), [sd["layer1.weight"], sd["layer1.bias"], sd["layer2.weight"], sd["layer2.bias"]])
    for name, g in zip(("l1w", "l1b", "l2w", "l2b"), grads):
        assert np.abs(ref[name][0] - g.numpy()).max() < 1e-11 and np.abs(g.numpy()).max() > 0, name
    assert (ref["l1w"][0][[3, 40]] == 0).all() and (ref["l1w"][1][[3, 40]] == 0).all()


@pytest.mark.parametrize("N", Q.TB_BWD_N)
def test_time_branch_float32_evaluation_meets_every_bound(N):
    W = Q.tb_weights(1, zero_rows=(0, 17, 63))
    t, _ = Q.tb_times(W, N, seed=1)
    fw, got = Q.tb_forward(W, t), Q.tb_eval32(W, t)
    assert got["pre"].dtype == np.float32 and got["tout"].dtype == np.float32
    assert Q.ratio(got["pre"], fw["pre"], fw["bpre"]) <= 1.0 and Q.ratio(got["tout"], fw["tout"][:, :30], fw["btout"][:, :30]) <= 1.0
    rng = np.random.default_rng(N)
    for S, with_dtp in ((5, True), (33, True), (70, True), (33, False)):
        dtout, dtp = Q.tb_cotangents(N, S, with_dtp, seed=N)
        pre = {k: rng.standard_normal(v.shape).astype(np.float32) for k, v in W.items()}
        ref = Q.tb_backward(W, t, S, dtout, dtp, pre)
        got = Q.tb_eval32(W, t, S, dtout, dtp, pre)
        assert ((got["pre"] > 0) == ref["gate"]).all()
        for name in ("l1w", "l1b", "l2w", "l2b"):
            assert got[name].dtype == np.float32 and Q.ratio(got[name], *ref[name]) <= 1.0, (S, with_dtp, name)


def test_gate_margin_of_every_generated_case():
    """the share of (ray, neuron) pairs that would have to be excluded is zero: every pre is 0 by construction or GATE_MARGIN bounds away"""
    for zero_rows in ((), (0, 17, 63)):
        W = Q.tb_weights(0, zero_rows)
        total = 0
        for N in Q.TB_BWD_N:
            t, redraws = Q.tb_times(W, N)
            total += redraws
            assert Q.gate_margin(W, t) >= Q.GATE_MARGIN and (np.abs(t) <= 1).all()
            fw = Q.tb_forward(W, t)
            assert (fw["pre"][:, list(zero_rows)] == 0).all() and (fw["bpre"][:, list(zero_rows)] == 0).all()
            if N >= 31:
                assert (fw["pre"] > 0).any(0).sum() > 40 and (fw["pre"] < 0).any(0).sum() > 40   # both sides of the gate are met
        assert total < 16, total   # a re-draw is rare: the margin is a few 1e-5 of pre's spread


@pytest.mark.parametrize("N", Q.TB_BWD_N)
@pytest.mark.parametrize("S", Q.TB_BWD_S)
def test_dtout_of_ray_against_per_sample_sums(N, S):
    rng = np.random.default_rng([N, S])
    per_sample = rng.integers(-4, 5, size=(N * S, 30)).astype(np.float64)
    dtout, dtp = Q.tile_records(per_sample, N, S)
    got, cond, cnt = Q.dtout_of_ray(dtout, dtp, N, S)
    assert np.array_equal(got, per_sample.reshape(N, S, 30).sum(1)) and np.isfinite(cond).all()
    t0, t1, slot = Q.ray_tiles(N, S)
    assert np.array_equal(cnt, t1 - t0 + 1)
    # the generator's NaN slots are exactly the ones the tile kernel leaves unwritten: nothing else may be read
    gd, gp = Q.tb_cotangents(N, S, True)
    assert np.array_equal(np.isnan(gd[:, :30]), np.isnan(dtout[:, :30])) and np.array_equal(np.isnan(gp[:, :, :30]), np.isnan(dtp[:, :, :30]))
    assert np.isnan(gd[:, 30:]).all() and np.isnan(gp[:, :, 30:]).all()
    gd0, gp0 = Q.tb_cotangents(N, S, False)
    assert gp0 is None and np.isfinite(gd0[:, :30]).all() and np.isfinite(Q.dtout_of_ray(gd0, None, N, S)[0]).all()
    if S in (32, 33) and N > 1:
        assert (slot == 0).sum() >= 1 and ((slot == 0) & (t1 > t0)).any() == (S > 32)   # a ray that starts exactly on a tile edge
