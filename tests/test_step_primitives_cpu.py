"""Keeps tests/_step_prim.py honest without a GPU: every float64 reference there against independent float64 evidence
(torch.optim.Adam, F.interpolate, torch autograd, index_put_, the oracle's eff_distloss / frame_depth_loss / tv_loss, the
reference's own TV vectors in tests/golden/tv.npz) to 1e-12 of the condition scale; every generator produces the regime it claims;
and the FLOAT32 torch / oracle evaluation of every case lies inside the bound test_gpu_step_primitives.py holds the kernels to, so
that no bound is tighter than a legitimate float32 ordering of the same arithmetic."""
import math
import os

import numpy as np
import pytest
import torch

import _step_prim as P
from _util import GOLDEN, record_margin
from oracle import rodynrf_oracle as O

EPS64 = 1e-12


def _agree(a, b, cond, tag, floor=0.0):
    a, b, cond = P.f64(a), P.f64(b), np.broadcast_to(P.f64(cond), np.shape(P.f64(b)))
    err = np.abs(a - b)
    assert (err <= EPS64 * cond + floor).all(), f"{tag}: float64 forms differ by {float((err / (cond + 1e-300)).max()):.2e} of the scale"


def _inside(got, ref, cond, k, tag, extra=0.0):
    r = P.error_ratio(got, ref, cond, k, extra)
    record_margin(tag, r)
    assert r <= 1.0, f"{tag}: the float32 evaluation sits at {r:.3f} of the bound"
    return r


# ---- Adam -------------------------------------------------------------------------------------------------------------------
def _adam_f32_torch(p, g, m, v, split, step, gs, lr0, lr1, beta1, beta2, eps):
    """torch.optim.Adam's single-tensor ordering in float32 (lerp_, mul_ + addcmul_, sqrt / sqrt(bc2) + eps, addcdiv_), with the
    hyper-parameters as the C ABI receives them (float32)"""
    f = lambda x: float(np.float32(x))
    p, g, m, v = [torch.from_numpy(np.array(a, np.float32)) for a in (p, g, m, v)]
    b1, b2 = f(beta1), f(beta2)
    g = g * f(gs)
    m = m.lerp(g, f(1.0 - b1))
    v = v.mul(b2).addcmul(g, g, value=f(1.0 - b2))
    denom = (v.sqrt() / f(math.sqrt(1.0 - b2 ** step))).add(f(eps))
    lr = torch.where(torch.arange(p.numel()) < split, torch.tensor(f(lr0)), torch.tensor(f(lr1)))
    p1 = p - (lr / f(1.0 - b1 ** step)) * (m / denom)
    return p1.numpy(), m.numpy(), v.numpy()


def test_adam_reference_is_torch_adam_in_float64():
    n, split = 1028, 512
    p, g, m, v, _ = P.adam_inputs(n, 0)
    a = torch.nn.Parameter(torch.from_numpy(p[:split]).double())
    b = torch.nn.Parameter(torch.from_numpy(p[split:]).double())
    opt = torch.optim.Adam([{"params": [a], "lr": 0.02}, {"params": [b], "lr": 1e-3}], betas=(0.9, 0.99), eps=1e-8)
    cur = dict(p=p, m=m, v=v)
    for step in (1, 2, 3):
        g = P.adam_inputs(n, step)[1]
        a.grad, b.grad = torch.from_numpy(g[:split]).double() * 0.5, torch.from_numpy(g[split:]).double() * 0.5
        opt.step()
        r = P.adam_ref(cur["p"], g, cur["m"], cur["v"], split, step, 0.5, f32_consts=False, **P.ADAM_HYPER)
        want = torch.cat([a, b]).detach().numpy()
        _agree(r["p"] - P.f64(cur["p"]), want - P.f64(cur["p"]), r["cond_upd"], f"step {step} update", floor=1e-15)
        st = opt.state[a]
        _agree(r["m"][:split], st["exp_avg"], r["cond_m"][:split], "m")
        _agree(r["v"][:split], st["exp_avg_sq"], r["cond_v"][:split], "v")
        cur = r


def test_adam_generators_and_float32_inside_bound():
    for n in P.ADAM_SIZES[:2]:
        p, g, m, v, z = P.adam_inputs(n, 0, "warm")
        nz = np.abs(g[g != 0])
        assert (g[z] == 0).all() and (m[z] == 0).all() and (v[z] == 0).all() and 2 <= z.size < n
        assert g[:2].all(), "non-zero gradients on the lr0 side of split = 4 at every size"
        if n > 4:   # (two non-zero elements cannot span the range)
            assert nz.min() < 1e-4 and nz.max() > 1e4 and nz.max() * 1.0 < 1e18
        assert P.adam_splits(n) == sorted({0, 4, n - 4, n})
        for state in ("zero", "warm"):
            for step in (1, 2, 1000):
                for gs in (1.0, 0.5):
                    for split in P.adam_splits(n):
                        p, g, m, v, z = P.adam_inputs(n, step, state)
                        r = P.adam_ref(p, g, m, v, split, step, gs, **P.ADAM_HYPER)
                        p1, m1, v1 = _adam_f32_torch(p, g, m, v, split, step, gs, **P.ADAM_HYPER)
                        tag = f"n={n} {state} step={step} gs={gs} split={split}"
                        _inside(m1, r["m"], r["cond_m"], P.K_ADAM_M, tag + " m")
                        _inside(v1, r["v"], r["cond_v"], P.K_ADAM_V, tag + " v")
                        _inside(P.f64(p1) - P.f64(p), r["upd"], r["cond_upd"], P.K_ADAM_UPD, tag + " update", P.half_ulp(r["p"]))
                        assert (r["upd"][z] == 0).all() and (p1[z] == p[z]).all()
    assert P.ADAM_SIZES[2] // 4 > 2048 * 256, "the largest size enters the grid-stride loop"


# ---- loss terms -------------------------------------------------------------------------------------------------------------
def _loss_torch(kind, norm, x, y, ysign, w, coef, dtype):
    x = torch.from_numpy(x).to(dtype).requires_grad_(True)
    y = None if y is None else torch.from_numpy(y).to(dtype).requires_grad_(True)
    r = x if y is None else x + ysign * y
    rho = r * r if kind == "square" else (r.abs() if kind == "abs" else r)
    if w is None:
        val = coef * rho.mean()
    else:
        wt = torch.from_numpy(w).to(dtype)
        t = (rho * wt[:, None]).sum()
        val = coef * (t / (wt.sum() + 1e-8) if norm == "weight" else t / x.numel())
    gs = torch.autograd.grad(val, [x] + ([] if y is None else [y]))
    return val.detach().numpy(), [a.numpy() for a in gs]


@pytest.mark.parametrize("shape", P.LOSS_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_loss_reference_and_float32_inside_bound(shape):
    rows, cols = shape
    for kind in P.LOSS_KINDS:
        for regime, norm, use_w, ysign in (("plain", "mean", False, -1.0), ("plain", "mean", True, 1.0), ("plain", "weight", True, -1.0),
                                           ("zero_w", "weight", True, -1.0), ("tie", "mean", True, -1.0)):
            x, y, w = P.loss_inputs(rows, cols, 0, regime)
            if regime == "plain" and rows > 4:
                assert (w == 0).any() and (w > 0).any()
            if regime == "zero_w":
                assert not w.any()
            if regime == "tie":
                assert (x == y).all()
            w_ = w if use_w else None
            r = P.loss_ref(kind, norm, x, y, ysign, w_, coef=0.7)
            tag = f"{kind} {regime} {norm} w={use_w}"
            v64, g64 = _loss_torch(kind, norm, x, y, ysign, w_, 0.7, torch.float64)
            # (torch adds the double 1e-8, the kernel the float32 one: a difference of 6e-17 in Z, visible only where Z is 1e-8)
            _agree(r["value"], v64, r["cond"] * (1e4 if regime == "zero_w" else 1.0), tag)
            _agree(r["gx"], g64[0], np.abs(r["gx"]) * (1e4 if regime == "zero_w" else 1.0), tag + " gx")
            _agree(r["gy"], g64[1], np.abs(r["gy"]) * (1e4 if regime == "zero_w" else 1.0), tag + " gy")
            v32, g32 = _loss_torch(kind, norm, x, y, ysign, w_, 0.7, torch.float32)
            _inside(v32, r["value"], r["cond"], P.k_loss(rows * cols), tag)
            _inside(g32[0], r["gx"], np.abs(r["gx"]), P.k_loss_grad(rows * cols), tag + " gx")
            if regime == "tie" and kind != "identity":
                assert not r["gx"].any() and r["value"] == 0, "residual exactly 0: value and gradient exactly 0"
            if regime == "zero_w":
                assert r["value"] == 0 and r["Z"] == float(np.float32(1e-8))
    sizes = [a * b for a, b in P.LOSS_SHAPES]
    assert {32767, 32768, 32769} <= set(sizes) and 10923 * 3 == 32769 and max(sizes) > 2 * P.LOSS_BLOCK_ELEMS


def test_loss_two_rank_statistics_recombine():
    x, y, w = P.loss_inputs(778, 3, 1)
    h = 389
    for kind in P.LOSS_KINDS:
        for norm in ("mean", "weight"):
            whole = P.loss_ref(kind, norm, x, y, -1.0, w, coef=1.3)
            gws = sum(P.loss_stats(kind, x[s], y[s], -1.0, w[s])[1] for s in (slice(0, h), slice(h, None)))
            halves = [P.loss_ref(kind, norm, x[s], y[s], -1.0, w[s], coef=1.3, global_ws=gws, world=2) for s in (slice(0, h), slice(h, None))]
            if norm == "mean":   # a plain mean of a half is over ITS element count: the mean over ranks is the global mean
                assert halves[0]["Z"] == h * 3
            # Z = global / world + 1e-8 on every rank: the recombined masked mean divides by sum w + 2e-8, not + 1e-8
            slack = 1.0 + (2e-8 / gws) / EPS64 if norm == "weight" else 1.0
            _agree(0.5 * (halves[0]["value"] + halves[1]["value"]), whole["value"], whole["cond"] * slack, f"{kind} {norm}", floor=1e-18)
            _agree(np.concatenate([halves[0]["gx"], halves[1]["gx"]]) / 2, whole["gx"], np.abs(whole["gx"]) * slack, f"{kind} {norm} gx",
                   floor=1e-18)


# ---- frame depth loss ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", P.FDL_BATCHES)
def test_frame_depth_reference_and_float32_inside_bound(N):
    for ties in (False, True):
        for use_mask in (False, True):
            pred, gt, frame, mask, T = P.fdl_inputs(N, 0, ties)
            counts = np.bincount(frame[(frame >= 0) & (frame < T)], minlength=T)
            assert tuple(counts[:7]) == P.fdl_frame_sizes(N) and counts[7] > 1 and (frame == T).sum() == 4 and (frame == -1).sum() == 4
            if ties:
                i = np.nonzero(frame == 5)[0]
                assert (pred[i] == np.sort(pred[i])[(i.size - 1) >> 1]).sum() >= 3
            mk = mask if use_mask else None
            r = P.fdl_ref(pred, gt, frame, T, mk, coef=0.04)
            for dtype, check in ((torch.float64, "agree"), (torch.float32, "inside")):
                p = torch.from_numpy(pred).to(dtype).requires_grad_(True)
                val = 0.04 * O.frame_depth_loss(p, torch.from_numpy(gt).to(dtype), torch.from_numpy(frame), T,
                                                mask=None if mk is None else torch.from_numpy(mk))
                g, = torch.autograd.grad(val, p)
                tag = f"N={N} ties={ties} mask={use_mask}"
                if check == "agree":
                    _agree(r["value"], val.detach(), r["cond"], tag)
                    _agree(r["grad"], g, r["gcond"], tag + " grad", floor=1e-18)
                else:
                    _inside(val.detach(), r["value"], r["cond"], P.k_fdl(N, T), tag)
                    _inside(g, r["grad"], r["gcond"], P.k_fdl_grad(N), tag + " grad")
            out = (frame < 0) | (frame >= T)
            assert not r["grad"][out].any() and not r["grad"][frame == 1].any(), "outside [0, T) and single-ray frames: exactly 0"
    r = P.fdl_ref(pred, gt, np.arange(N) % 2000 + 5, 4000, None)
    assert r["count"] == 0 and np.isnan(r["value"]), "every frame skipped: the reference is 0 / 0"


# ---- distortion loss ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", P.DIST_SIZES)
def test_distloss_reference_and_float32_inside_bound(S):
    w, m, iv = P.dist_inputs(S, 0)
    assert not w[0].any() and (w[1] != 0).sum() == 1 and w[2, S - 1] == 1 and (np.diff(m, axis=-1) >= 0).all()
    if S >= 16:
        assert (np.diff(m[3]) == 0).sum() >= 7 * (S // 8)
    for interval in (float(np.float32(1.0 / S)), iv):
        r = P.dist_ref(w, m, interval)
        for dtype in (torch.float64, torch.float32):
            wt = torch.from_numpy(w).to(dtype).requires_grad_(True)
            it = torch.from_numpy(interval).to(dtype) if isinstance(interval, np.ndarray) else interval
            rays = torch.stack([O.eff_distloss(wt[n:n + 1], torch.from_numpy(m[n:n + 1]).to(dtype),
                                               it[n:n + 1] if torch.is_tensor(it) else it) for n in range(w.shape[0])])
            g, = torch.autograd.grad(rays.sum(), wt)
            if dtype == torch.float64:
                _agree(r["ray"], rays.detach(), r["cond"], f"S={S}")
                _agree(r["grad"], g, r["gcond"], f"S={S} grad")
                pub = O.eff_distloss_published_grad(wt.detach(), torch.from_numpy(m).double(), it) * w.shape[0]
                assert np.abs(P.f64(pub) - r["grad"]).max() <= 1e-12, "the published prefix form, float64"
            else:
                _inside(rays.detach(), r["ray"], r["cond"], P.k_dist(S), f"S={S}")
                _inside(g, r["grad"], r["gcond"], P.k_dist_grad(S), f"S={S} grad")
        assert r["ray"][0] == 0 and not r["grad"][0].any()


# ---- TV -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", P.TV_SHAPES, ids=str)
def test_tv_reference_and_float32_inside_bound(shape):
    C, H, W = shape
    x, pre = P.tv_inputs(C, H, W, 0)
    ch, cw = 0.37, 1.9
    r = P.tv_ref(x, ch, cw)
    for dtype in (torch.float64, torch.float32):
        t = torch.from_numpy(x).to(dtype)[None].requires_grad_(True)
        sh = ((t[:, :, 1:] - t[:, :, :-1]) ** 2).sum()
        sw = ((t[:, :, :, 1:] - t[:, :, :, :-1]) ** 2).sum()
        g, = torch.autograd.grad(ch * sh + cw * sw, t)
        if dtype == torch.float64:
            _agree(r["sums"], [sh.item(), sw.item()], r["sums"], str(shape))
            _agree(r["grad"], g[0], r["gcond"], f"{shape} grad")
            if H > 1 and W > 1:   # the oracle's tv_loss: 2 (h_tv / count_h + w_tv / count_w)
                want = 2 * (r["sums"][0] / (C * (H - 1) * W) + r["sums"][1] / (C * H * (W - 1)))
                assert abs(O.tv_loss(t.detach()).item() - want) <= EPS64 * want
        else:
            _inside([sh.item(), sw.item()], r["sums"], r["sums"], P.k_tv_sum(C, H, W), str(shape))
            _inside(g[0], r["grad"], r["gcond"], P.K_TV_G + 2, f"{shape} grad")          # the GPU file's bound through TVLoss ...
            want = P.f64(pre) + r["grad"]                                                   # ... and into a pre-filled gradient
            _inside(torch.from_numpy(pre) + g[0], want, r["gcond"], P.K_TV_G, f"{shape} grad +=", P.half_ulp(want))
    if H == 1:
        assert r["sums"][0] == 0
    for layout in P.TV_LAYOUTS:
        v = P.tv_tensor(x, layout)
        assert torch.equal(v[0], torch.from_numpy(x))
        if layout == "cl_h" and H > 1 and W > 1:
            assert v.stride(3) > v.stride(2)
        if layout == "cf" and H * W > 1:
            assert v.stride(1) != 1


def test_tv_reference_matches_the_reference_fixture():
    """tests/golden/tv.npz holds the reference's own TVLoss values and gradients (float32) on a plane, a line and a row, for
    ignore_axis None / "h" / "w": the float64 sums and gradient formula reproduce them to float32 resolution"""
    tv = np.load(os.path.join(GOLDEN, "tv.npz"))
    seen = 0
    for nm in ("plane", "line", "row"):
        x = tv[f"t.{nm}.x"]
        _, C, H, W = x.shape
        for ax in ("None", "h", "w"):
            ch = 0.0 if ax == "h" else (2.0 / (C * (H - 1) * W) if H > 1 else math.nan)
            cw = 0.0 if ax == "w" else (2.0 / (C * H * (W - 1)) if W > 1 else math.nan)
            if math.isnan(ch) or math.isnan(cw):
                continue   # a zero count: the reference's value is 0 / 0
            r = P.tv_ref(x[0], ch, cw)
            want = ch * r["sums"][0] + cw * r["sums"][1]
            assert abs(float(tv[f"t.{nm}.v.{ax}"]) - want) <= 4e-6 * want, (nm, ax)
            g = tv[f"t.{nm}.g.{ax}"].astype(np.float64)[0]
            assert np.abs(g - r["grad"]).max() <= 4e-6 * np.abs(r["grad"]).max(), (nm, ax)
            seen += 1
    assert seen >= 5


# ---- dense L1 -------------------------------------------------------------------------------------------------------------------
def _l1_torch(fs, act, dtype):
    ts = [torch.from_numpy(a).to(dtype).requires_grad_(True) for a in fs]
    p0, p1, p2, l0, l1, l2 = ts
    f = torch.einsum("cyx,cz->xyz", p0, l0) + torch.einsum("czx,cy->xyz", p1, l1) + torch.einsum("czy,cx->xyz", p2, l2)
    val = (torch.relu(f) if act == "relu" else torch.nn.functional.softplus(f + P.L1_SHIFT)).abs().mean()
    return val.detach().numpy(), [g.numpy() for g in torch.autograd.grad(1.7 * val, ts)]


@pytest.mark.parametrize("grid", P.L1_GRIDS, ids=str)
def test_dense_l1_reference_and_float32_inside_bound(grid):
    for act in ("relu", "softplus"):
        for regime in ("normal", "integer"):
            fs, pre = P.l1_inputs(grid, 0, regime)
            r = P.l1_ref(fs, act, g=1.7)
            if regime == "integer":
                assert (r["f"] == np.round(r["f"])).all() and r["n_flip"] == 0
                if min(grid) > 1:
                    assert (r["f"] == 0).any(), "voxels with f == 0 exactly"
            v64, g64 = _l1_torch(fs, act, torch.float64)
            v32, g32 = _l1_torch(fs, act, torch.float32)
            _agree(r["value"], v64, r["cond"], f"{grid} {act} {regime}")
            _inside(v32, r["value"], r["cond"], P.k_l1(grid), f"{grid} {act} {regime}")
            for i in range(6):
                # (F.softplus is the identity beyond its threshold 20, slope exactly 1; the kernel's and the reference's slope is
                # the sigmoid, 1 - 2.1e-9 there)
                _agree(r["grads"][i], g64[i], r["gconds"][i] * (1.0 if act == "relu" else 1.0 + 2.1e-9 / EPS64), f"{grid} {act} {regime} g{i}",
                       floor=1e-18)
                _inside(g32[i], r["grads"][i], r["gconds"][i], P.k_l1(grid, True), f"{grid} {act} {regime} g{i}", r["flips"][i])


# ---- upsample -------------------------------------------------------------------------------------------------------------------
def test_upsample_reference_and_float32_inside_bound():
    for (hi, ho) in P.UP_PAIRS:
        for (wi, wo) in P.UP_PAIRS:
            x = P.rng(8, hi, wi).standard_normal((4, hi, wi)).astype(np.float32)
            r = P.up_ref(x, ho, wo)
            f32 = torch.nn.functional.interpolate(torch.from_numpy(x)[None], size=(ho, wo), mode="bilinear", align_corners=True)[0]
            _inside(f32, r["out"], r["cond"], P.K_UP, f"{hi}x{wi} -> {ho}x{wo}", r["lam"])
            if all(a == 1 or b == 1 or (a - 1) / (b - 1) == float(np.float32(a - 1) / np.float32(b - 1)) for a, b in ((hi, ho), (wi, wo))):
                f64_ = torch.nn.functional.interpolate(torch.from_numpy(x).double()[None], size=(ho, wo), mode="bilinear", align_corners=True)[0]
                _agree(r["out"], f64_, r["cond"], f"{hi}x{wi} -> {ho}x{wo}")   # scales exact in float32: the same indices
            if (hi, wi) == (ho, wo) or {hi, ho} | {wi, wo} <= {1, 5}:
                assert not r["lam"].any(), "exact products and lambda 0: no allowance"
            if (hi, wi) == (ho, wo):
                assert np.array_equal(r["out"], x.astype(np.float64)) and r["pin"].all(), "identity resize"
            # pinned points: ATen's float32 lambda is exactly 0 on both axes, the output is the source texel bit for bit
            assert r["pin"][0, 0] and np.array_equal(f32.numpy()[:, r["pin"]], r["src"][:, r["pin"]].astype(np.float32))
            assert np.array_equal(r["out"][:, r["pin"]], r["src"][:, r["pin"]])
    below = P.up_pinned_below(157, 133)
    assert 121 in below and 0 < below.min(), "157 -> 133: rounded src integral, exact product below it, strictly inside at 121"
    x = P.rng(8, 157, 7).standard_normal((4, 157, 7)).astype(np.float32)
    assert P.up_ref(x, 133, 7)["pin"][121].all() and P.up_ref(x, 133, 7)["lam"][:, 121].max() > 0
    assert not any(P.up_pinned_below(a, b).size for a, b in P.UP_PAIRS[:6]), "none of the other pairs has such a point"


# ---- rows_scatter_add -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", P.RSA_CASES, ids=str)
def test_rows_scatter_reference_is_index_put(case):
    R, C, N = case
    idx, g, pre = P.rsa_inputs(R, C, N, 0)
    if N >= 8:
        assert (idx < 0).any() and (idx >= R).any()
    ok = (idx >= 0) & (idx < R)
    want = torch.from_numpy(pre).double().index_put_((torch.from_numpy(idx[ok]),), torch.from_numpy(g[ok]).double(), accumulate=True)
    ref = P.rsa_ref(idx, g, pre)
    assert np.array_equal(ref, want.numpy()) and np.array_equal(ref, ref.astype(np.float32)) and np.abs(ref).max() < 2 ** 24
    assert (R * C <= P.RSA_LDS_FLOATS) == (case != (683, 12, 3000) and case != (8193, 1, 5000))
