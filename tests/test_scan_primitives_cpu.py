"""The float64 reference of the per-field ray scan (tests/_scan_prim.py) checked on the CPU: its written-out backward (the source
of the condition scales) against torch autograd, its forward against the oracle's raw2alpha on _dists_viewdirs, both against plain
per-ray Python loops, and the redraw cap of the seeded regimes."""
import math

import pytest
import torch

import _scan_prim as Q
from oracle import rodynrf_oracle as O

N = Q.N_RAYS
KEYS = ("gsig", "gf", "g_z", "g_rays")


def _rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


@pytest.mark.parametrize("regime", Q.REGIMES)
def test_written_out_backward_matches_autograd(regime):
    for S in (1, 2, 33, 65, 129):
        for act, rt, scale in (("relu", "ndc", 25.0), ("softplus", "contract", 1.0), ("softplus", "world", 25.0)):
            for cs in Q.COT_SETS:
                r = Q.reference(regime, N, S, act, rt, scale, cs)
                x = r["x"]
                c = {k: (None if v is None else v.double()) for k, v in r["cot"].items()}
                w = Q.backward(x["rays"].double(), x["z"].double(), x["valid"], x["raw"].double(), act, rt, scale,
                               gw=c["w"], gs=c["s"], gd=c["d"])
                for k in KEYS:
                    assert bool(torch.isfinite(w[k]).all()), (regime, S, act, rt, cs, k)
                    assert _rel(w[k], r["grads"][k]) <= 1e-12, (regime, S, act, rt, cs, k, _rel(w[k], r["grads"][k]))
                    # a condition scale bounds the quantity it belongs to (up to the float64 rounding of 1 - alpha behind a wall)
                    slack = 1e-12 * float(r["grads"][k].abs().max()) + 1e-300
                    assert bool((r["gcond"][k] * (1 + 1e-12) + slack >= r["grads"][k].abs()).all()), (regime, S, act, rt, cs, k)
                if rt == "world":
                    assert not bool(r["grads"]["g_rays"].any())
                else:
                    assert not bool(r["grads"]["g_rays"][:, :3].any())


@pytest.mark.parametrize("regime", Q.REGIMES)
def test_forward_matches_the_oracle(regime):
    for S in Q.SIZES:
        for rt, scale in (("ndc", 25.0), ("contract", 1.0), ("world", 25.0)):
            r = Q.reference(regime, N, S, "relu", rt, scale)
            x = r["x"]
            dists, _ = O._dists_viewdirs(x["rays"].double(), x["z"].double(), rt)
            alpha, weight, _ = O.raw2alpha(x["sigma"].double(), dists * scale)
            assert _rel(r["fwd"]["ds"], dists * scale) <= 1e-15
            assert _rel(r["fwd"]["w"], weight.double()) <= 1e-12 or float(weight.abs().max()) == 0.0
            assert _rel(r["fwd"]["alpha"], alpha.double()) <= 1e-12 or float(alpha.abs().max()) == 0.0


def test_regimes_hold_what_they_promise():
    for S in Q.SIZES + (Q.S_MAX,):
        n = 3 if S == Q.S_MAX else N
        for act in Q.ACTS:
            for regime in Q.REGIMES:
                x = Q.generate(regime, n, S, act)
                assert Q.REDRAWS[(regime, n, S, act, Q.SEED)] <= 0.10, (regime, S, act)
                assert bool((x["z"][:, 1:] >= x["z"][:, :-1]).all())
            x = Q.generate("act_edges", n, S, act)
            kink = 0.0 if act == "relu" else 20.0 - Q.SHIFT
            d = (x["raw"].double() - kink)
            assert float(d.abs().min()) >= Q.c_ops(S, 32, act == "softplus") * Q.EPS32
            assert bool((d > 0).any()) and bool((d < 0).any())
        v = Q.generate("invalid", n, S)["valid"]
        assert not bool(v[0].any())
        if S > 1 and n > 2:
            assert bool(v[2].any()) and not bool(v[2].all())
        x = Q.generate("wall", n, S)
        q = Q.forward(x["rays"].double(), x["z"].double(), x["sigma"].double(), "ndc", 25.0)
        assert S == 1 or float((x["sigma"].double() * q["ds"]).max()) >= 17.0, "an opaque sample (S = 1 has no interval)"
        # both sides of every 32-sample edge hold an opaque sample on some ray (S = 4096: the sweep's 255 rays); the last sample, which
        # has no interval, is never the wall
        ne = Q.edge_sweep_rays(S) if S == Q.S_MAX else n
        assert ne >= Q.edge_sweep_rays(S)
        for regime in ("wall", "double_wall"):
            x = Q.generate(regime, ne, S)
            q = Q.forward(x["rays"].double(), x["z"].double(), x["sigma"].double(), "ndc", 25.0)
            opaque = (x["sigma"].double() * q["ds"] >= 17.0).any(0)
            for k in range(1, (S - 1) // 32 + 1):
                assert 32 * k - 1 >= S - 1 or bool(opaque[32 * k - 1]), (regime, S, 32 * k - 1)
                assert 32 * k >= S - 1 or bool(opaque[32 * k]), (regime, S, 32 * k)
            assert S == 1 or bool(opaque[0])
        if S == Q.S_MAX:   # the N = 3 case: last lane of the first tile, first lane of the second
            assert [Q.wall_position(i, S) for i in range(3)] == [0, 31, 32]
        if S >= 64:   # dists of order 1 / S: the optical depth of a thin ray is of order 1 at every S
            x = Q.generate("thin", n, S)
            q = Q.forward(x["rays"].double(), x["z"].double(), x["sigma"].double(), "ndc", 25.0)
            tau = (x["sigma"].double() * q["ds"]).sum(-1)
            assert 0.1 < float(tau.min()) and float(tau.max()) < 2.0


def _loops(rays, z, valid, raw, act, rt, scale, gw, gs, gd):
    """one ray, plain Python floats"""
    S = len(z)
    d = rays[3:6]
    nrm = 1.0 if rt == "world" else math.sqrt(sum(v * v for v in d))
    sig, dact = [], []
    for j in range(S):
        if act == "relu":
            a, g = max(raw[j], 0.0), 1.0 if raw[j] > 0 else 0.0
        else:
            t = raw[j] + Q.SHIFT
            a, g = (t, 1.0) if t > 20.0 else (math.log1p(math.exp(t)), 1.0 / (1.0 + math.exp(-t)))
        sig.append(a if valid[j] else 0.0)
        dact.append(g)
    dz = [z[j + 1] - z[j] if j + 1 < S else 0.0 for j in range(S)]
    ds = [v * nrm * scale for v in dz]
    e = [math.exp(-sig[j] * ds[j]) for j in range(S)]
    alpha = [1.0 - v for v in e]
    p = [1.0 - a + 1e-10 for a in alpha]
    T, w = [], []
    t = 1.0
    for j in range(S):
        T.append(t)
        w.append(alpha[j] * t)
        t *= p[j]
    gsig, gf, g_z, g_nrm = [0.0] * S, [0.0] * S, [0.0] * S, 0.0
    for k in range(S):
        suf = sum(gw[m] * w[m] for m in range(k + 1, S))
        g_alpha = gw[k] * T[k] - suf / p[k]
        gsig[k] = gs[k] + g_alpha * ds[k] * (1.0 - alpha[k])
        gf[k] = gsig[k] * dact[k] if valid[k] else 0.0
        g_ds = gd[k] + g_alpha * sig[k] * (1.0 - alpha[k])
        g_nrm += g_ds * dz[k] * scale
        if k + 1 < S:
            g_z[k] -= g_ds * nrm * scale
            g_z[k + 1] += g_ds * nrm * scale
    g_rays = [0.0] * 6
    if rt != "world":
        for i in range(3):
            g_rays[3 + i] = g_nrm * d[i] / nrm
    return w, ds, gsig, gf, g_z, g_rays


def test_reference_matches_plain_per_ray_loops():
    for regime, S, act, rt, scale in (("wall", 5, "relu", "ndc", 25.0), ("invalid", 33, "softplus", "contract", 1.0),
                                      ("act_edges", 7, "softplus", "world", 25.0), ("mixed", 65, "relu", "contract", 25.0),
                                      ("double_wall", 9, "relu", "ndc", 1.0), ("act_edges", 6, "relu", "ndc", 25.0)):
        r = Q.reference(regime, 6, S, act, rt, scale, ("w", "s", "d"))
        x = r["x"]
        for n in range(6):
            args = [x[k][n].double().tolist() for k in ("rays", "z")] + [x["valid"][n].tolist(), x["raw"][n].double().tolist()]
            cot = [r["cot"][k][n].double().tolist() for k in ("w", "s", "d")]
            w, ds, gsig, gf, g_z, g_rays = _loops(*args, act, rt, scale, *cot)
            # the forward entry's sigma is the fp32 rounding of act(raw): the loops' weights follow the backward side's sigma
            sig = torch.where(x["valid"][n].bool(), Q.density_act(x["raw"][n].double(), act), torch.zeros(S, dtype=torch.float64))
            q = Q.forward(x["rays"][n:n + 1].double(), x["z"][n:n + 1].double(), sig[None], rt, scale)
            for got, ref in ((w, q["w"][0]), (ds, q["ds"][0]), (gsig, r["grads"]["gsig"][n]), (gf, r["grads"]["gf"][n]),
                             (g_z, r["grads"]["g_z"][n]), (g_rays, r["grads"]["g_rays"][n])):
                got = torch.tensor(got, dtype=torch.float64)
                assert float((got - ref).abs().max()) <= 1e-11 * max(float(ref.abs().max()), 1e-300), (regime, S, n)


def test_operation_count_is_the_compositors_plus_the_written_differences():
    import _comp_prim as P
    for S in (1, 64, 257, 4096):
        assert Q.c_ops(S, 64, False) == P.c_ops(S) + 5 * S
        assert Q.c_ops(S, 32, False) == P.c_ops(S) + 5 * S + S // 32 - S // 64
        assert Q.c_ops(S, 64, True) == P.c_ops(S) + 10 * S
