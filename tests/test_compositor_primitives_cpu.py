"""The compositor's float64 reference and input regimes (tests/_comp_prim.py), checked without a GPU:
  * fixture pin: on the compositor inputs the reference generated (tests/golden/<case>.npz: fs.rgb, fs.sigma, fd.*) the
    float64 reference reproduces the outputs the reference produced (c0.* / c1.*) at test_golden_forward's tolerances;
  * the written-out float64 backward equals autograd to 1e-12 of each gradient's maximum, and every condition scale is at
    least |gradient| element by element;
  * every regime x size: gate margins, the redraw cap, the exact-0 / exact-1 cases exact in float32 and float64, the regime's
    defining property, and the float32 ORACLE inside the bound the GPU test holds the kernels to (the inputs are fair to a
    correct fp32 implementation).  RDRF_MARGINS records the float32-oracle ratios under the same check names as the GPU test."""
import numpy as np
import pytest
import torch

import _comp_prim as P
from _util import CASES, FWD_ELEM, assert_close, load_case, record_margin

N = P.N_RAYS
BIG = {"wall": (4096,), "mixed": (4096,)}


def _sizes(regime):
    return P.SIZES + BIG.get(regime, ())


@pytest.mark.parametrize("case", CASES)
def test_float64_reference_reproduces_the_reference_generated_compositor_fixtures(case):
    g, *_ = load_case(case)
    rt = str(g["meta.ray_type"])
    x32 = dict(rgb_s=g["fs.rgb"], sigma_s=g["fs.sigma"], rgb_d=g["fd.rgb"], sigma_d=g["fd.sigma"], dists=g["fd.dists"],
               blending=g["fd.blending"], z_vals=g["fd.z"], rays=g["rays"])
    x32 = {k: torch.from_numpy(np.array(v)) for k, v in x32.items()}
    for white, pre in ((False, "c0."), (True, "c1.")):
        outs, _ = P.oracle_run(x32, white, rt)
        for k, v in zip(P.ONAMES, outs):
            assert v.dtype == torch.float64
            at = 256.0 * 2.0 ** -22 if (rt == "contract" and "depth" in k) else 0.0
            assert_close(v, g[pre + k], pre + k, atol=at, elem=FWD_ELEM)


@pytest.mark.parametrize("regime", P.REGIMES)
def test_written_out_backward_equals_autograd_and_condition_scales_dominate(regime):
    for S in _sizes(regime):
        for white, rt in ((False, "ndc"), (True, "ndc"), (True, "contract"), (False, "world")):
            r = P.reference(regime, N, S, white, rt, "all")
            man = P.backward(P.widen(r["x"]), [c.double() for c in r["cot"]], white, rt)
            none = P.expected_none("all", rt)
            for k, name in enumerate(P.INAMES):
                assert (r["grads"][k] is None) == none[k], (name, S, rt)
                if r["grads"][k] is None:
                    assert float(man[k].abs().max()) == 0.0
                    continue
                ga = r["grads"][k]
                assert bool(torch.isfinite(ga).all()), (name, S)
                rel = float((ga - man[k]).abs().max() / max(float(ga.abs().max()), 1e-300))
                assert rel <= 1e-12, f"{regime} S={S} {rt} white={white} d/d{name}: written-out vs autograd {rel:.2e}"
                assert bool((r["gcond"][k] >= ga.abs() * (1 - 1e-12)).all()), f"{regime} S={S} d/d{name}: condition scale < |g|"
            for k in range(13):
                assert bool((r["fcond"][k] >= r["outs"][k].abs() * (1 - 1e-12)).all()), (P.ONAMES[k], S)


@pytest.mark.parametrize("cot_set", P.COT_SETS, ids=lambda s: "+".join(P.ONAMES[i] for i in s))
def test_autograd_none_pattern_is_the_data_flow_table(cot_set):
    """which inputs get no gradient from one cotangent (or a trainer pair): autograd on the oracle = expected_none"""
    for rt in P.RAY_TYPES:
        r = P.reference("mixed", N, 65, True, rt, cot_set)
        assert [g is None for g in r["grads"]] == P.expected_none(cot_set, rt), (cot_set, rt)
        man = P.backward(P.widen(r["x"]), [None if c is None else c.double() for c in r["cot"]], True, rt)
        for k, ga in enumerate(r["grads"]):
            if ga is None:
                assert float(man[k].abs().max()) == 0.0, (P.INAMES[k], cot_set)
            else:   # against the condition scale: d acc_map_d / d anything is a pure cancellation, ~1e-10 / U of its terms
                assert float((ga - man[k]).abs().max()) <= 1e-12 * float(r["gcond"][k].max())


def _alpha(sig, dist, dtype):
    return 1.0 - torch.exp(-(sig.to(dtype) * dist.to(dtype)))


@pytest.mark.parametrize("regime", P.REGIMES)
def test_generators(regime):
    for S in _sizes(regime) + ((4097,) if regime == "wall" else ()):
        x = P.generate(regime, N, S)
        assert all(v.dtype == torch.float32 and bool(torch.isfinite(v).all()) for v in x.values())
        assert x["sigma_d"].shape == (N, S) and x["rgb_s"].shape == (N, S, 3) and x["rays"].shape == (N, 6)
        # gate margins and the redraw cap (asserted in the generator too)
        assert float(P.gate_margins(x).min()) >= P.gate_margin(regime, S), (regime, S)
        assert P.REDRAWS[(regime, N, S, P.SEED)] <= N // 10
        xd_d, xd_s = x["sigma_d"] * x["dists"], x["sigma_s"] * x["dists"]
        a32 = (_alpha(x["sigma_d"], x["dists"], torch.float32), _alpha(x["sigma_s"], x["dists"], torch.float32))
        if regime == "thin":
            assert float(max(xd_d.max(), xd_s.max())) <= 0.03 * (1 + 1e-6) and float(min(xd_d.min(), xd_s.min())) > 0
        if regime == "mixed":
            for s in (x["sigma_d"], x["sigma_s"]):
                nz = s[s > 0]
                assert 0.55 <= float((s == 0).float().mean()) <= 0.85 or S <= 2
                assert float(nz.min()) >= 1e-3 * (1 - 1e-6) and float(nz.max()) <= 1e3 * (1 + 1e-6)
        if regime == "wall":
            kinds = set()
            for n in range(N):
                pd, ps = P.wall_positions(n, S)
                assert float(xd_d[n, pd]) > 17 and float(a32[0][n, pd]) == 1.0, "dynamic wall: alpha rounds to 1 in fp32"
                if ps != pd:
                    assert float(xd_s[n, ps]) > 17 and float(a32[1][n, ps]) == 1.0
                assert int((a32[0][n] == 1).sum()) == 1
                kinds.add("first" if pd % 64 == 0 else ("last" if pd % 64 == 63 else "mid"))
                if pd >= 64 * ((S - 1) // 64):
                    kinds.add("last_tile")
            if S >= 65:
                assert {"first", "last", "last_tile"} <= kinds, kinds
        if regime == "double_wall" and S >= 2:
            run = (a32[0] == 1).sum(-1)
            assert int(run.min()) >= 2 or S < 3, "two or more opaque dynamic samples in a row"
            if S >= 8:
                assert int(run.max()) >= 5
            assert not bool(((a32[0] == 1) & (a32[1] == 1)).any())
        if regime in ("empty_d", "empty_both"):
            assert float(x["sigma_d"].abs().max()) == 0.0
        if regime in ("empty_s", "empty_both"):
            assert float(x["sigma_s"].abs().max()) == 0.0
        if regime == "blend_edges":
            b = x["blending"]
            assert bool((b[0::4] == 0).all()) and bool((b[1::4] == 1).all())
            assert bool(((b[2::4] == 0) | (b[2::4] == 1)).all())
            assert int(((b != 0) & (b != 1)).sum()) <= N // 4, "only the gate-holding sample of the opaque rays is off the edges"
            if S >= 2:
                assert bool((b[2::4][:, 0] != b[2::4][:, 1]).all()), "alternating samples"
        if regime == "gates":
            q = P._pieces(P.widen(x), True, "world")
            assert float(min(x["rgb_s"].min(), x["rgb_d"].min())) < -0.3 and float(max(x["rgb_s"].max(), x["rgb_d"].max())) > 1.5
            pre = torch.cat([q["Rf"], q["Rs"], q["Rd"]], -1)
            assert bool((pre < 0).any()) or S > 2
            assert bool((pre > 1).any())
            assert bool((~q["rl_on"]).any()), "some ray has acc_map_full > 1: the relu gate is off"
            assert float(x["blending"].min()) < 0 or float(x["blending"].max()) > 1
        # the exact cases hold in float32 as well as in float64
        for white in (False, True):
            o64, _ = P.oracle_run(x, white, "world")
            o32, _ = P.oracle_run(x, white, "world", dtype=torch.float32)
            want = 1.0 if white else 0.0
            if regime == "empty_both":
                for k in (0, 4, 8):
                    assert bool((o64[k] == want).all()) and bool((o32[k] == want).all()), (P.ONAMES[k], S)
            if regime == "empty_d":
                assert bool((o64[8] == want).all()) and bool((o32[8] == want).all())
            if regime == "empty_s":
                assert bool((o64[4] == want).all()) and bool((o32[4] == want).all())
            # no gate of the float32 oracle is decided differently from the float64 one
            q64 = P._pieces(P.widen(x), white, "world")
            q32 = P._pieces({k: v.clone() for k, v in x.items()}, white, "world")
            for key in ("Rf", "Rs", "Rd"):
                assert torch.equal((q64[key] >= 0) & (q64[key] <= 1), (q32[key] >= 0) & (q32[key] <= 1)), (key, S, white)
            assert torch.equal(q64["rl_on"], q32["rl_on"]), (S, white)
        if regime == "double_wall":
            for k in (3, 7, 11):
                w = o64[k].abs()
                assert not bool(((w > 0.9999e-30) & (w < 1.0001e-30)).any()), "no reference weight on the 1e-30 line"
                assert bool((w < 1e-30).any()) or S < 5 or k == 3   # (the full factor of a one-field wall is ~blending)


@pytest.mark.parametrize("regime", P.REGIMES)
def test_float32_oracle_is_inside_the_bound(regime):
    """the oracle in float32 (torch's own cumprod / sum and their autograd) against the float64 reference, all cotangents,
    at the bound of the GPU test: a correct fp32 implementation can meet it"""
    for S in _sizes(regime):
        for white, rt in ((False, "ndc"), (True, "ndc"), (True, "contract"), (False, "world")):
            r = P.reference(regime, N, S, white, rt, "all")
            o32, g32 = P.oracle_run(r["x"], white, rt, r["cot"], torch.float32)
            tag = f"{regime} S={S} {rt} white={int(white)}"
            for k, name in enumerate(P.ONAMES):
                ratio = P.error_ratio(o32[k], r["outs"][k], r["fcond"][k], S, P.out_atol(k, rt))
                record_margin(f"{tag} {name}", ratio)
                assert ratio <= 1.0, f"{tag} {name}: float32 oracle at {ratio:.3f} of the bound"
            for k, name in enumerate(P.INAMES):
                if r["grads"][k] is None:
                    assert g32[k] is None
                    continue
                ratio = P.error_ratio(g32[k], r["grads"][k], r["gcond"][k], S)
                record_margin(f"{tag} d/d{name}", ratio)
                assert ratio <= 1.0, f"{tag} d/d{name}: float32 oracle at {ratio:.3f} of the bound"
