"""The compositor on inputs of its own: rodynrf.raw2outputs (k_composite / composite_body, k_composite_bwd and the need[...]
pruning of _CompositeFn.backward) against the float64 reference of tests/_comp_prim.py, on the regimes the fields' own outputs
never reach: opaque samples at tile edges, runs of them (T underflows), an empty dynamic / static / both fields (U = 0),
blending exactly 0 / 1, colour maps outside [0, 1], acc_map_full > 1.

Shapes: N = 24 rays (16 + 8), S in {1, 2, 63, 64, 65, 128, 129, 257} for every regime, S = 4096 for `wall` and `mixed` (all 64
carry slots of the backward), S = 4097 for the backward's loud error.

Bound of EVERY comparison (derived in tests/_comp_prim.py):
    max|err| <= 1e-4 max|ref| + c(S) 2^-23 max(condition scale),   c(S) = 6 S + S / 64 + 32
(6 rounded operations per factor of the longest transmittance product, S / 64 + 6 levels of a per-ray sum, 26 for the per-sample
arithmetic), plus test_golden_forward's 256 * 2^-22 on the contract depth maps.  The float32 oracle meets the same bound on the
same cases (test_compositor_primitives_cpu.py); profiles/compositor_primitives_margins.txt holds both sets of ratios."""
import pytest
import torch

import _comp_prim as P
from _util import record_margin

pytestmark = pytest.mark.gpu

N = P.N_RAYS
COMBOS = ((False, "ndc"), (True, "ndc"), (True, "contract"), (False, "world"))


def _inputs(x32, grad=True):
    return [x32[k].cuda().requires_grad_(grad) for k in P.INAMES]


def _run(x32, white, rt, cot=None, coin=False, ins=None):
    """raw2outputs on the GPU; cot: list of 13 fp32 cotangents (None entries: none) -> (outs, grads with None kept)"""
    import rodynrf
    ins = _inputs(x32) if ins is None else ins
    w = torch.tensor([1.0 if white else 0.0], device="cuda") if coin else bool(white)
    outs = rodynrf.raw2outputs(*ins, is_train=True, ray_type=rt, add_white_bg=w)
    assert len(outs) == 13
    if cot is None:
        return outs, None
    sel = [k for k in range(13) if cot[k] is not None]
    g = torch.autograd.grad([outs[k] for k in sel], ins, [cot[k].cuda() for k in sel], allow_unused=True)
    torch.cuda.synchronize()
    return outs, list(g)


def _check(got, ref, cond, S, tag, atol=0.0, rows=None):
    got = got.detach().cpu()
    assert bool(torch.isfinite(got).all()), f"{tag}: NaN / Inf"
    if rows is not None:
        got, ref, cond = got[rows], ref[rows], cond[rows]
    ratio = P.error_ratio(got, ref, cond, S, atol)
    record_margin(tag, ratio)
    assert ratio <= 1.0, f"{tag}: max|err| is {ratio:.3f} x (1e-4 max|ref| + c 2^-23 max cond)"


def _check_outs(outs, r, S, rt, tag):
    for k, name in enumerate(P.ONAMES):
        _check(outs[k], r["outs"][k], r["fcond"][k], S, f"{tag} {name}", P.out_atol(k, rt))


def _check_grads(grads, r, S, rt, tag, strict_none):
    for k, name in enumerate(P.INAMES):
        if r["grads"][k] is None:
            if strict_none:
                assert grads[k] is None, f"{tag}: d/d{name} is {'a zero' if not grads[k].any() else 'a'} tensor, autograd gives None"
            else:   # rays outside NDC: None or zero
                assert grads[k] is None or float(grads[k].abs().max()) == 0.0, f"{tag}: d/d{name} must be None or zero"
            continue
        assert grads[k] is not None, f"{tag}: d/d{name} is None"
        _check(grads[k], r["grads"][k], r["gcond"][k], S, f"{tag} d/d{name}")


def _bit_equal(a, b, tag):
    for k, (u, v) in enumerate(zip(a, b)):
        assert (u is None) == (v is None), (tag, k)
        if u is not None:
            assert torch.equal(u, v), f"{tag}: entry {k} differs"


@pytest.mark.parametrize("regime", P.REGIMES)
def test_forward_matches_float64(regime):
    """a + e: the 13 outputs for every size, ray type and background; the device coin is bit-equal to the host bool"""
    for S in P.SIZES:
        x = P.generate(regime, N, S)
        for rt in P.RAY_TYPES:
            for white in (False, True):
                r = P.reference(regime, N, S, white, rt)
                with torch.no_grad():
                    outs, _ = _run(x, white, rt, ins=_inputs(x, False))
                    coin, _ = _run(x, white, rt, coin=True, ins=_inputs(x, False))
                tag = f"{regime} S={S} {rt} white={int(white)}"
                _check_outs(outs, r, S, rt, tag)
                _bit_equal(outs, coin, tag + " device coin")
                if regime == "empty_both":   # exactly 0.0 / exactly 1.0 before the clamp, in either precision
                    for k in (0, 4, 8):
                        assert bool((outs[k] == (1.0 if white else 0.0)).all()), (tag, P.ONAMES[k])
                if regime == "double_wall":  # behind the walls: exactly 0 or below 1e-30 wherever the reference is
                    for k in (3, 7, 11):
                        tiny = r["outs"][k].abs() < 1e-30
                        assert bool((outs[k].cpu().abs()[tiny] < 1e-30).all()), (tag, P.ONAMES[k])


@pytest.mark.parametrize("regime", P.REGIMES)
def test_backward_all_cotangents_matches_float64(regime):
    """b + e: seeded cotangents on all 13 outputs, every input gradient; rays: checked for NDC, None or zero otherwise"""
    for S in P.SIZES:
        for white, rt in COMBOS:
            r = P.reference(regime, N, S, white, rt, "all")
            outs, grads = _run(r["x"], white, rt, r["cot"])
            tag = f"{regime} S={S} {rt} white={int(white)}"
            _check_outs(outs, r, S, rt, tag)
            _check_grads(grads, r, S, rt, tag, strict_none=False)
            if rt == "ndc":
                assert grads[7] is not None and bool((grads[7][:, [0, 1, 3, 4]] == 0).all())
                assert torch.equal(grads[7][:, 2], grads[7][:, 5])
            if S in (2, 65):
                _, gc = _run(r["x"], white, rt, r["cot"], coin=True)
                _bit_equal(grads, gc, tag + " device coin")


@pytest.mark.parametrize("regime", ["wall", "mixed"])
def test_4096_samples_use_every_carry_slot(regime):
    S = 4096
    r = P.reference(regime, N, S, True, "ndc", "all")
    if regime == "wall":
        pos = [P.wall_positions(n, S)[0] for n in range(N)]
        assert max(pos) >= 64 * 63, "a wall in the last tile"
    outs, grads = _run(r["x"], True, "ndc", r["cot"])
    _check_outs(outs, r, S, "ndc", f"{regime} S={S}")
    _check_grads(grads, r, S, "ndc", f"{regime} S={S}", strict_none=False)


def test_4097_samples_backward_refuses_loudly_and_forward_still_matches():
    S = 4097
    r = P.reference("wall", N, S, True, "contract")
    ins = _inputs(r["x"])
    outs, _ = _run(r["x"], True, "contract", ins=ins)
    _check_outs(outs, r, S, "contract", f"wall S={S}")
    with pytest.raises(Exception, match="S <= 4096"):
        outs[0].sum().backward()
    torch.cuda.synchronize()


@pytest.mark.parametrize("cot_set", P.COT_SETS, ids=lambda s: "+".join(P.ONAMES[i] for i in s))
def test_backward_one_cotangent_at_a_time(cot_set):
    """c: one output's cotangent (or a pair the trainer uses: rgb_map_s + depth_map_s, depth_map_d + weights_d; dynamicness
    alone is among the singles).  An input autograd gives None must come back None -- not a zero tensor -- and the others match."""
    cases = [(g, 65, True, "ndc") for g in P.REGIMES] + [("mixed", 1, False, "contract"), ("mixed", 257, True, "world"),
                                                         ("wall", 129, False, "ndc")]
    for regime, S, white, rt in cases:
        r = P.reference(regime, N, S, white, rt, cot_set)
        assert [g is None for g in r["grads"]] == P.expected_none(cot_set, rt)
        _, grads = _run(r["x"], white, rt, r["cot"])
        _check_grads(grads, r, S, rt, f"{regime} S={S} {rt} cot={'+'.join(P.ONAMES[i] for i in cot_set)}", strict_none=True)
    s = set(cot_set)
    none = P.expected_none(cot_set, "ndc")
    assert none[5] == (not (s & {0, 1, 2, 3, 12})), "blending: None from the static-only and dynamic-only maps"
    assert none[0] == (not (s & {0, 4})), "rgb_s: None unless rgb_map_full or rgb_map_s carries a cotangent"


@pytest.mark.parametrize("regime", ["gates", "empty_both"])
def test_clamp_and_relu_gates(regime):
    """d: the gated rays only.  A colour cotangent behind a closed clamp gate gives EXACTLY 0.0; at the exact boundaries
    (empty_both: pre-clamp maps exactly 0.0 / 1.0) torch's clamp passes the gradient and so must the kernel; where
    acc_map_full > 1 the relu gate is closed and neither the background nor the far plane sends a gradient."""
    col_in = {0: (0, 2), 4: (0,), 8: (2,)}          # rgb map -> the colour inputs it reads
    for S in P.SIZES:
        for white, rt in ((False, "world"), (True, "ndc")):
            x64 = P.widen(P.generate(regime, N, S))
            q = P._pieces(x64, white, rt)
            for k, key in ((0, "Rf"), (4, "Rs"), (8, "Rd")):
                r = P.reference(regime, N, S, white, rt, (k,))
                _, grads = _run(r["x"], white, rt, r["cot"])
                closed = (q[key] < 0) | (q[key] > 1)                      # [N,3]
                tag = f"{regime} S={S} {rt} white={int(white)} cot={P.ONAMES[k]}"
                for i in col_in[k]:
                    g = grads[i].cpu()
                    assert bool((g.permute(0, 2, 1)[closed] == 0.0).all()), f"{tag}: d/d{P.INAMES[i]} behind a closed gate"
                if regime == "empty_both":
                    assert not bool(closed.any()) and bool(((q[key] == 0) | (q[key] == 1)).all())
                    rows = torch.ones(N, dtype=torch.bool)
                else:
                    rows = closed.any(-1)
                if bool(rows.any()):
                    for i, name in enumerate(P.INAMES):
                        if r["grads"][i] is not None:
                            _check(grads[i], r["grads"][i], r["gcond"][i], S, f"{tag} gated rays d/d{name}", rows=rows)
            if regime == "gates":
                off = ~q["rl_on"]
                assert bool(off.any())
                for cs in ((0,), (1,)):
                    r = P.reference(regime, N, S, white, rt, cs)
                    _, grads = _run(r["x"], white, rt, r["cot"])
                    for i, name in enumerate(P.INAMES):
                        if r["grads"][i] is not None:
                            _check(grads[i], r["grads"][i], r["gcond"][i], S,
                                   f"{regime} S={S} {rt} white={int(white)} cot={P.ONAMES[cs[0]]} relu-off rays d/d{name}", rows=off)
                    if cs == (1,) and rt == "ndc":
                        assert bool((grads[7].cpu()[off] == 0).all()), "far plane behind a closed relu gate"


@pytest.mark.parametrize("regime", ["mixed", "wall"])
def test_non_contiguous_and_expanded_inputs_are_bit_equal(regime):
    """f: sigma in transposed storage, z_vals from expand (one row for all rays): same bits as their contiguous copies"""
    for S in (65, 129):
        x = P.generate(regime, N, S)
        x["z_vals"] = x["z_vals"][:1].expand(N, S).contiguous()
        cot = P.cotangents(N, S, 7)
        base = _run(x, True, "ndc", cot)
        ins = _inputs(x)
        for i in (1, 3):
            t = x[P.INAMES[i]].cuda().t().contiguous().t().requires_grad_(True)
            assert not t.is_contiguous() or S == 1
            ins[i] = t
        zrow = x["z_vals"][:1].cuda().requires_grad_(True)
        ins[6] = zrow.expand(N, S)
        outs = _run(x, True, "ndc", ins=ins)[0]
        sel = list(range(13))
        g = torch.autograd.grad([outs[k] for k in sel], ins[:6] + [zrow, ins[7]], [cot[k].cuda() for k in sel])
        _bit_equal(base[0], outs, f"{regime} S={S} outputs")
        for i in (0, 1, 2, 3, 4, 5, 7):
            assert torch.equal(base[1][i], g[i]), f"{regime} S={S}: d/d{P.INAMES[i]} differs for the strided inputs"
        # the expanded row's gradient is the column sum of the per-ray one
        ref = base[1][6].double().sum(0, keepdim=True)
        assert float((g[6].double() - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
