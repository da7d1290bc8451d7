"""No GPU: keeps tests/_warp_prim.py honest (the references, generators and bounds of test_gpu_warp_primitives.py).
  * each reference equals torch autograd in float64 over a forward written out here (X0 = PE(xn) with fixed gate masks, xw =
    (x - lo) inv - 1, the three layers), on consistent inputs, to 1e-12 relative;
  * each reference equals plain integer loops on an exact case;
  * a plain float32 evaluation (eval32) meets every bound at every shape the GPU file uses, on exact, dense and gate_edges inputs;
  * the exact generators' 2^24 assertion holds at every count the GPU file uses;
  * the mutation table: every wrong kernel of _warp_prim.MUTATIONS, as a variant of eval32, exceeds a bound on the dense case."""
import numpy as np
import pytest
import torch

import _warp_prim as Q
from _util import pkg

f32, f64 = np.float32, np.float64


def _wl():
    return Q.warp_layout(pkg())


def _sl():
    return Q.sf_layout(pkg())


def test_layouts_are_consistent():
    wl, sl = _wl(), _sl()
    spans = sorted([(int(wl["in3"][:63].min()), 63), (int(wl["in3"][63:].min()), 30), (int(wl["H3"].min()), 64), (int(wl["H4"].min()), 64)])
    assert all(a + n <= b for (a, n), (b, _) in zip(spans, spans[1:])) and spans[-1][0] + 64 <= wl["rows"]
    assert wl["DX0"] + 64 <= wl["grows"] and wl["SM"] + 3 <= wl["grows"]
    assert len(set(sl["X"].tolist())) == 36 and sl["X"].max() < sl["H0"].min() and sl["H4"].max() < sl["rows"]
    inv = Q.box_inv(Q.BOX_POW2)
    assert inv.dtype == f32 and inv.tolist() == [0.5, 1.0, 0.25] and len(set(Q.box_inv(Q.BOX_ODD).tolist())) == 3


# ---- autograd ----------------------------------------------------------------------------------------------------------------------
def _pe(x, F):
    """[n][3] -> [n][6 F]: sin(2^f x_d), d-major, then cos likewise"""
    q = torch.stack([x[:, d] * 2.0 ** f for d in range(3) for f in range(F)], -1)
    return torch.cat([torch.sin(q), torch.cos(q)], -1)


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300))


@pytest.mark.parametrize("box", [Q.BOX_ODD, Q.BOX_POW2], ids=["odd", "pow2"])
def test_warp_reference_against_autograd(box):
    lay = _wl()
    c = Q.warp_case(lay, "dense", 3, 13, seed=2, box=box)
    n = 39
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=f64))
    lo, inv = t(c["box"][0]), t(Q.box_inv(c["box"]))
    rng = np.random.default_rng(1)
    x = (t(rng.uniform(-0.9, 0.9, size=(n, 3))) / inv + (t(c["box"][0]) + t(c["box"][1])) / 2).requires_grad_(True)
    tout = t(rng.standard_normal((n, 30))).requires_grad_(True)
    W3, W4, W5 = (t(c["W"][k]) for k in ("l3", "l4", "l5"))
    a = Q.samples(c["act"], n)
    M3, M4 = t(a[:, lay["H3"]] > 0), t(a[:, lay["H4"]] > 0)
    xn = (x - lo) * inv - 1
    X0 = torch.cat([xn, _pe(xn, 10)], -1)
    h3 = M3 * (torch.cat([X0, tout], -1) @ W3.T)
    h4 = M4 * (h3 @ W4.T)
    delta = h4 @ W5.T
    delta.retain_grad()
    xp = x + delta
    xw = (xp - lo) * inv - 1
    hX = t(Q.samples(c["grw"], n)[:, lay["DX0"] + lay["in3"][:63] - lay["x0_row0"]])   # what the heads hand down, per X0 column
    loss = (t(c["dxw"]) * xw).sum() + (t(c["dxn"]) * xn).sum() + (t(c["gp"]) * xp).sum() + (hX * X0).sum()
    loss.backward()
    # the case's saved X0 rows are this graph's own values (float64 kept: the reference widens whatever it is handed)
    c = dict(c, act=c["act"].astype(f64), pre=None)
    Q.put_rows(c["act"], lay["in3"][:63], X0.detach().numpy())
    r = Q.warp_reference(c, lay)
    assert _rel(r["g_xyz"][0], x.grad.numpy()) < 1e-12
    assert _rel(r["dd"][0][:n], delta.grad.numpy()) < 1e-12 and not r["dd"][0][n:].any()
    assert _rel(r["dtout"][0], tout.grad.numpy().reshape(3, 13, 30).sum(1)) < 1e-12


@pytest.mark.parametrize("box", [Q.BOX_ODD, Q.BOX_POW2], ids=["odd", "pow2"])
def test_scene_flow_reference_against_autograd(box):
    lay = _sl()
    n = 37
    c = Q.sf_case(lay, "dense", n, seed=2, box=box, prefill=False)
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=f64))
    lo, inv = t(c["box"][0]), t(Q.box_inv(c["box"]))
    rng = np.random.default_rng(1)
    x = (t(rng.uniform(-0.9, 0.9, size=(n, 3))) / inv + (t(c["box"][0]) + t(c["box"][1])) / 2).requires_grad_(True)
    tt = t(rng.uniform(-1, 1, size=(n, 1)))
    a = Q.samples(c["rows"], n)
    M0, M2, M4 = (t(a[:, lay[k]] > 0) for k in ("H0", "H2", "H4"))
    W = [t(w) for w in c["W"]]
    xn = (x - lo) * inv - 1
    qt = torch.cat([tt * 2.0 ** f for f in range(4)], -1)
    X = torch.cat([xn, _pe(xn, 4), tt, torch.sin(qt), torch.cos(qt)], -1)
    out = (M4 * ((M2 * ((M0 * (X @ W[0].T)) @ W[1].T)) @ W[2].T)) @ W[3].T
    ((t(c["gf"]) * out[:, :3]).sum() + (t(c["gb"]) * out[:, 3:]).sum()).backward()
    c = dict(c, rows=c["rows"].astype(f64))
    Q.put_rows(c["rows"], lay["X"], X.detach().numpy())
    assert _rel(Q.sf_reference(c, lay)["g_pts"][0], x.grad.numpy()) < 1e-12


# ---- integer loops -------------------------------------------------------------------------------------------------------------------
def test_warp_reference_against_plain_loops():
    """units: dd, dz, dX0, e, dn in quarters; g_xyz in sixteenths (inv = (2, 4, 1) quarters)"""
    lay = _wl()
    c = Q.warp_case(lay, "exact", 2, 21, seed=1)
    inv4 = [int(4 * v) for v in Q.box_inv(c["box"])]
    assert inv4 == [2, 4, 1]
    W = {k: v.astype(np.int64) for k, v in c["W"].items()}
    in3, H3, H4 = lay["in3"], lay["H3"], lay["H4"]
    g16 = np.zeros((42, 3), dtype=np.int64)
    dd4 = np.zeros((42, 3), dtype=np.int64)
    dt4 = np.zeros((2, 30), dtype=np.int64)
    for i in range(42):
        tl, s = divmod(i, 32)
        col, gcol = c["act"][tl, :, s].astype(np.int64), c["grw"][tl, :, s].astype(np.int64)
        dxw, dxn, gp, pre = (c[k][i].astype(np.int64) for k in ("dxw", "dxn", "gp", "pre"))
        dd = [int(dxw[d]) * inv4[d] + 4 * int(gp[d]) for d in range(3)]
        dz4 = [sum(int(W["l5"][o, k]) * dd[o] for o in range(3)) if col[H4[k]] > 0 else 0 for k in range(64)]
        dz3 = [sum(int(W["l4"][o, k]) * dz4[o] for o in range(64)) if col[H3[k]] > 0 else 0 for k in range(64)]
        dX = [4 * int(gcol[lay["DX0"] + in3[cc] - lay["x0_row0"]]) + sum(int(W["l3"][o, cc]) * dz3[o] for o in range(64)) for cc in range(63)]
        for e in range(30):
            dt4[i // 21, e] += sum(int(W["l3"][o, 63 + e]) * dz3[o] for o in range(64))
        for d in range(3):
            acc = dX[d]
            for f in range(10):
                j = 10 * d + f
                acc += (1 << f) * (dX[3 + j] * int(col[in3[33 + j]]) - dX[33 + j] * int(col[in3[3 + j]]))
            dn = 4 * int(dxn[d]) + acc + 4 * int(dxw[d])
            g16[i, d] = 16 * int(pre[d]) + dn * inv4[d] + 16 * int(gp[d])
        dd4[i] = dd
    r = Q.warp_reference(c, lay)
    assert np.array_equal(r["g_xyz"][0] * 16, g16.astype(f64)) and np.abs(g16).max() > 1000
    assert np.array_equal(r["dd"][0][:42] * 4, dd4.astype(f64)) and not r["dd"][0][42:].any()
    assert np.array_equal(r["dtout"][0] * 4, dt4.astype(f64)) and np.abs(dt4).max() > 0


@pytest.mark.parametrize("variant", ["both", "f", "b"])
def test_scene_flow_reference_against_plain_loops(variant):
    lay = _sl()
    n = 34
    c = Q.sf_case(lay, "exact", n, seed=1, gf=variant != "b", gb=variant != "f")
    inv4 = [int(4 * v) for v in Q.box_inv(c["box"])]
    W = [w.astype(np.int64) for w in c["W"]]
    g4 = np.zeros((n, 3), dtype=np.int64)
    for i in range(n):
        tl, s = divmod(i, 32)
        col = c["rows"][tl, :, s].astype(np.int64)
        dz = [0] * 6
        if c["gf"] is not None:
            dz[:3] = [int(v) for v in c["gf"][i]]
        if c["gb"] is not None:
            dz[3:] = [int(v) for v in c["gb"][i]]
        for layer, key in ((3, "H4"), (2, "H2"), (1, "H0")):
            dz = [sum(int(W[layer][o, k]) * dz[o] for o in range(len(dz))) if col[lay[key][k]] > 0 else 0 for k in range(64)]
        dX = [sum(int(W[0][o, cc]) * dz[o] for o in range(64)) for cc in range(36)]
        for d in range(3):
            acc = dX[d]
            for f in range(4):
                j = 4 * d + f
                acc += (1 << f) * (dX[3 + j] * int(col[lay["X"][15 + j]]) - dX[15 + j] * int(col[lay["X"][3 + j]]))
            g4[i, d] = 4 * int(c["pre"][i, d]) + acc * inv4[d]
    r = Q.sf_reference(c, lay)
    assert np.array_equal(r["g_pts"][0] * 4, g4.astype(f64)) and np.abs(g4).max() > 4 * 4


# ---- eval32 meets every bound; the exact generators' assertion ----------------------------------------------------------------------
def _warp_ratios(c, lay, mut=()):
    r, got = Q.warp_reference(c, lay), Q.warp_eval32(c, lay, mut)
    return {k: Q.ratio(got[k], *r[k]) for k in ("g_xyz", "dd", "dtout")}


def _sf_ratio(c, lay, mut=()):
    return Q.ratio(Q.sf_eval32(c, lay, mut)["g_pts"], *Q.sf_reference(c, lay)["g_pts"])


@pytest.mark.parametrize("gp", [True, False])
@pytest.mark.parametrize("N,S", Q.WARP_EXACT)
def test_warp_exact_generator_and_eval32(N, S, gp):
    lay = _wl()
    for box in (Q.BOX_POW2, Q.BOX_UNIT):
        c = Q.warp_case(lay, "exact", N, S, seed=int(gp), box=box, gp=gp)
        assert c["max_quanta"] < 2 ** 24
        r, got = Q.warp_reference(c, lay), Q.warp_eval32(c, lay)
        for k in ("g_xyz", "dd", "dtout"):   # exact: the float32 evaluation has the reference's very bits
            assert np.array_equal(got[k].astype(f64), r[k][0]), k


@pytest.mark.parametrize("kind,enc", [("dense", "normal"), ("dense", "sincos"), ("gate_edges", "normal")])
@pytest.mark.parametrize("N,S", Q.WARP_DENSE)
def test_warp_eval32_meets_every_bound(N, S, kind, enc):
    lay = _wl()
    for gp in (True, False):
        c = Q.warp_case(lay, kind, N, S, box=Q.BOX_ODD, enc=enc, gp=gp)
        rat = _warp_ratios(c, lay)
        assert all(v <= 1.0 for v in rat.values()), rat
    if kind == "gate_edges":
        a = Q.samples(c["act"], N * S)
        for key in ("H3", "H4"):
            assert set(np.unique(a[:, lay[key]].view(np.uint32)).tolist()) == set(Q.GATES.view(np.uint32).tolist())


@pytest.mark.parametrize("n", Q.SF_EXACT)
def test_scene_flow_exact_generator_and_eval32(n):
    lay = _sl()
    for seed, (gf, gb) in enumerate(((True, True), (True, False), (False, True))):
        c = Q.sf_case(lay, "exact", n, seed=seed, gf=gf, gb=gb)
        assert c["max_quanta"] < 2 ** 24
        assert np.array_equal(Q.sf_eval32(c, lay)["g_pts"].astype(f64), Q.sf_reference(c, lay)["g_pts"][0])
        c = Q.sf_case(lay, "exact", n, seed=seed, gf=gf, gb=gb, box=Q.BOX_ODD, prefill=False)
        e = Q.sf_reference(c, lay)["e"][0]
        assert np.array_equal(e, np.rint(e)) and np.array_equal(Q.sf_eval32(c, lay)["g_pts"], e.astype(f32) * Q.box_inv(Q.BOX_ODD)[None, :])


@pytest.mark.parametrize("kind,enc", [("dense", "normal"), ("dense", "sincos"), ("gate_edges", "normal")])
def test_scene_flow_eval32_meets_every_bound(kind, enc):
    lay = _sl()
    for gf, gb in ((True, True), (True, False), (False, True)):
        c = Q.sf_case(lay, kind, Q.SF_DENSE, box=Q.BOX_ODD, enc=enc, gf=gf, gb=gb)
        assert _sf_ratio(c, lay) <= 1.0


# ---- the mutation table: why each GPU assertion is there -----------------------------------------------------------------------------
@pytest.mark.parametrize("enc", ["normal", "sincos"])
@pytest.mark.parametrize("mut", Q.WARP_MUTATIONS)
def test_warp_mutations_exceed_the_bound(mut, enc):
    lay = _wl()
    c = Q.warp_case(lay, "dense", *Q.WARP_DENSE[1], box=Q.BOX_ODD, enc=enc)
    rat = _warp_ratios(c, lay, (mut,))
    print(mut, enc, rat)
    assert max(rat.values()) > 1.0, rat
    if mut != "no_inv_dd" and mut != "swap_inv":   # everything behind dd is caught by g_xyz
        assert rat["g_xyz"] > 1.0
    else:
        assert rat["dd"] > 1.0


@pytest.mark.parametrize("enc", ["normal", "sincos"])
@pytest.mark.parametrize("mut", Q.SF_MUTATIONS)
def test_scene_flow_mutations_exceed_the_bound(mut, enc):
    lay = _sl()
    c = Q.sf_case(lay, "dense", 37 * 32 - 5, box=Q.BOX_ODD, enc=enc)
    rat = _sf_ratio(c, lay, (mut,))
    print(mut, enc, rat)
    assert rat > 1.0, rat
