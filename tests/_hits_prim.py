"""Float64 reference of the surface hits (rdrf_hits_from_planes / rdrf_render_hits_fwd, include/rodynrf.h), on top of the
visibility reference of tests/_track_vis_prim.py; shared by test_hits_cpu.py and test_gpu_hits.py.  No GPU.

    T_s = prod_{i < s} F_i(dists_i)  (T_0 = 1, T_S the product after the last sample),  m_s = min_{i <= s} T_i,  L = 1 - tau
    j     = the first s with m_{s+1} <= L;  none: a miss
    d_hit = the root of m_j F_j(d) = L in [0, dists_j] (0 where m_j <= L already), by 200 bisection steps
    z_hit = z_j + d_hit / dists_j (z_{j+1} - z_j),   slope = |dT/dz| there

The arrays are fp32 numbers widened to float64, so both sides see the same values; L is 1 - tau rounded once in fp32."""
import numpy as np
import torch

import _track_vis_prim as P
from _util import record_margin

U24 = 2.0 ** -24
# ---- the residual bound of the GPU tests (test_gpu_hits.py has the count) ----------------------------------------------
C_FACTOR = 16      # units of 2^-24 in one factor F_s(dists_s), absolute: _track_vis_prim's 14 + 2 for dists formed in fp32
C0 = 40            # the solver's last step and what surrounds it, see test_gpu_hits.py


TAUS = {1: (0.5,), 3: (0.1, 0.5, 0.9), 8: (0.05, 0.1, 0.25, 0.5, 0.75, 0.9, 0.95, 0.99)}   # each a subset of the last
SHAPES_S, SHAPES_N = (1, 2, 63, 64, 65, 129), (1, 3, 257)
DISTANCE_SCALE = {"ndc": 25.0, "contract": 1.0}
# the depth check is asserted where the transmittance falls by at least this share of m_j across the hit interval
# (slope * (z_{j+1} - z_j) >= SLOPE_FLOOR * m_j): below it z_hit is ill-conditioned, a rounding of T moves it across the interval
SLOPE_FLOOR = 1e-3
FLOOR_CAP = 0.10   # at most this share of the hitting rays may lie under the floor


def planes(rt, N, S, seed=0):
    """seeded fp32 inputs of rdrf_hits_from_planes: rays [N,6], z, sigma_s, sigma_d, blending [N,S].  The optical depth of a
    sample is log-uniform over 1e-4 .. 5 times a per-ray scale of 1e-3 .. 1, so crossings lie anywhere from the first sample to
    beyond the last, at walls and in thin media; a fifth of the samples have one sigma exactly 0, blending is exactly 0 or 1
    in 15 % of the samples each."""
    g = torch.Generator().manual_seed(1000 * S + 10 * N + (0 if rt == "ndc" else 1) + 7919 * seed)
    o = torch.empty(N, 3).uniform_(-1.0, 1.0, generator=g)
    d = torch.randn(N, 3, generator=g)
    d = d / d.norm(dim=-1, keepdim=True) * torch.empty(N, 1).uniform_(0.5, 2.0, generator=g)
    w = 0.5 + torch.rand(N, max(S - 1, 1), generator=g)
    c = torch.cat([torch.zeros(N, 1), torch.cumsum(w, -1) / w.sum(-1, keepdim=True)], -1)[:, :S]
    z = c if rt == "ndc" else 0.05 + 20.0 * c ** 2
    rays = torch.cat([o, d], -1).float()
    z = z.float()
    dists = dists_of(z, rays, DISTANCE_SCALE[rt])
    x = 10.0 ** torch.empty(N, S).uniform_(-4.0, 0.7, generator=g) * 10.0 ** torch.empty(N, 1).uniform_(-3.0, 0.0, generator=g)
    sig = (x.double() / dists.clamp(min=1e-6)).float()
    kind = torch.rand(N, S, generator=g)
    sigma_s = torch.where(kind < 0.2, torch.zeros_like(sig), sig * torch.rand(N, S, generator=g))
    sigma_d = torch.where(kind > 0.8, torch.zeros_like(sig), sig * torch.rand(N, S, generator=g))
    b = torch.rand(N, S, generator=g)
    kb = torch.rand(N, S, generator=g)
    b = torch.where(kb < 0.15, torch.zeros_like(b), torch.where(kb > 0.85, torch.ones_like(b), b))
    return rays, z, sigma_s, sigma_d, b


def level(tau):
    """L = 1 - tau rounded once in fp32, as a float"""
    return float(np.float32(1.0) - np.float32(tau))


def dists_of(z, rays, distance_scale):
    """(z_{s+1} - z_s) |d| distance_scale, the last 0, in float64 from the fp32 inputs"""
    z, rays = torch.as_tensor(np.asarray(z)).double(), torch.as_tensor(np.asarray(rays)).double()
    w = torch.cat([z[:, 1:] - z[:, :-1], torch.zeros_like(z[:, :1])], -1)
    return w * rays[:, 3:].norm(dim=-1, keepdim=True) * float(distance_scale)


def dfactor(sigma_s, sigma_d, b, d):
    """dF/dd of _track_vis_prim.factor"""
    e_d, e_s = torch.exp(-sigma_d * d), torch.exp(-sigma_s * d)
    u, v = 1.0 - (1.0 - e_d) * b, 1.0 - (1.0 - e_s) * (1.0 - b)
    return -(b * sigma_d * e_d) * v - u * ((1.0 - b) * sigma_s * e_s)


def running_min(dists, sigma_s, sigma_d, blending):
    """(F [N,S], T [N,S+1], m [N,S+1]) in float64; T_S = the product after the last sample.  A NaN factor makes every T
    behind it NaN; m skips NaN (the callers look at the NaN's position themselves)"""
    dists, sigma_s, sigma_d, blending = (torch.as_tensor(np.asarray(t)).double() for t in (dists, sigma_s, sigma_d, blending))
    F = P.factor(sigma_s, sigma_d, blending, dists)
    T = torch.cumprod(torch.cat([torch.ones_like(F[:, :1]), F], -1), -1)
    m = torch.cummin(torch.where(torch.isnan(T), torch.full_like(T, float("inf")), T), -1).values
    return F, T, m


def hits(z, dists, sigma_s, sigma_d, blending, tau):
    """one level -> dict of [N] float64 / long / bool tensors: j (-1: miss or NaN), hit, nan, z, d, slope, m_j, and the
    reference's own F, T, m"""
    z, dists, sigma_s, sigma_d, blending = (torch.as_tensor(np.asarray(t)).double() for t in (z, dists, sigma_s, sigma_d, blending))
    N, S = z.shape
    L = level(tau)
    F, T, m = running_min(dists, sigma_s, sigma_d, blending)
    crossed = m[:, 1:] <= L                                     # [N,S]: sample s has m_{s+1} <= L
    any_cross = crossed.any(-1)
    j = torch.where(any_cross, crossed.double().argmax(-1), torch.full((N,), -1, dtype=torch.long))
    bad = torch.isnan(F)
    first_nan = torch.where(bad.any(-1), bad.double().argmax(-1), torch.full((N,), S, dtype=torch.long))
    nan = (first_nan < S) & (~any_cross | (first_nan <= j))
    hit = any_cross & ~nan
    jj = j.clamp(min=0)
    g = lambda t: t.gather(1, jj[:, None])[:, 0]
    mj, dj, ss, sd, b = g(m[:, :-1]), g(dists), g(sigma_s), g(sigma_d), g(blending)
    zj = g(z)
    zn = g(torch.cat([z[:, 1:], z[:, -1:]], -1))
    lo, hi = torch.zeros(N, dtype=torch.float64), dj.clone()
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        above = mj * P.factor(ss, sd, b, mid) > L
        lo, hi = torch.where(above, mid, lo), torch.where(above, hi, mid)
    d = torch.where(mj <= L, torch.zeros_like(hi), hi)
    frac = torch.where(dj > 0, d / dj.clamp(min=1e-300), torch.zeros_like(d))
    zh = zj + frac * (zn - zj)
    slope = mj * dfactor(ss, sd, b, d).abs() * torch.where(zn > zj, dj / (zn - zj).clamp(min=1e-300), torch.zeros_like(dj))
    zh = torch.where(hit, zh, z[:, -1])
    zh = torch.where(nan, torch.full_like(zh, float("nan")), zh)
    a_d, a_s = 1.0 - torch.exp(-sd * dj), 1.0 - torch.exp(-ss * dj)
    den = a_d * b + a_s * (1.0 - b)
    owner = torch.where(hit & (den != 0), a_d * b / torch.where(den != 0, den, torch.ones_like(den)), torch.zeros_like(den))
    return dict(j=torch.where(hit, j, torch.full_like(j, -1)), hit=hit, nan=nan, z=zh, d=d, slope=torch.where(hit, slope, torch.zeros_like(slope)),
                m_j=mj, owner=owner, den=den, F=F, T=T, m=m, L=L)


def residual_k(F, s):
    """k of the bound  k 2^-24 max(L, m_j)  for a crossing in sample s [N] (test_gpu_hits.py has the count): every factor in
    front of s carries C_FACTOR units ABSOLUTE, which is C_FACTOR / F_i relative to the product; a carry multiply per round
    of 64; C0 for the solver's last step"""
    inv = torch.cumsum(1.0 / F.clamp(min=1e-30), -1)
    inv = torch.cat([torch.zeros_like(inv[:, :1]), inv], -1)     # inv[:, s] = sum_{i < s} 1 / F_i
    s = s.clamp(min=0)
    return C_FACTOR * inv.gather(1, s[:, None])[:, 0] + (torch.div(s, 64, rounding_mode="floor") + 1).double() + C0


def clear_of_every_crossing(r):
    """[N] bool: the reference's m_{s+1} stays away from L by more than the residual bound at EVERY sample, so a kernel within
    that bound must find the same j and the same hit flag"""
    F, m, L = r["F"], r["m"], r["L"]
    N, S = F.shape
    ok = torch.ones(N, dtype=torch.bool)
    for s in range(S):
        k = residual_k(F, torch.full((N,), s, dtype=torch.long))
        ok &= ((m[:, s + 1] - L).abs() > k * U24 * torch.maximum(m[:, s], torch.full_like(m[:, s], L))) | torch.isnan(F).any(-1)
    return ok


def ulp32(x):
    """the spacing of fp32 numbers at |x| (float64 tensor in, float64 out)"""
    x32 = torch.as_tensor(np.asarray(x)).double().abs().float()
    return (torch.nextafter(x32, torch.full_like(x32, float("inf"))) - x32).double()


def check_against_reference(rt, pl, got, taus, tag, scale=None):
    """the residual, depth, bracket, flag and owner checks of one call against the float64 reference; returns the worst
    residual / bound"""
    rays, z, ss, sd, b = pl
    N, S = z.shape
    dists = dists_of(z, rays, DISTANCE_SCALE[rt] if scale is None else scale)
    z64 = z.double()
    worst, n_hit, n_floor, n_clear, n_all = 0.0, 0, 0, 0, 0
    for k, tau in enumerate(taus):
        r = hits(z, dists, ss, sd, b, tau)
        zk, hk = got["z"][k].cpu(), got["hit"][k].cpu()
        clear = clear_of_every_crossing(r)
        n_clear += int(clear.sum())
        n_all += N
        # flags and j exact wherever the reference is clear of every crossing
        assert bool((hk == r["hit"])[clear].all()), (tag, tau)
        miss = clear & ~r["hit"]
        assert bool((zk[miss] == z[miss, -1]).all()) and bool((got["owner"][k].cpu()[miss] == 0).all())
        sel = clear & r["hit"]
        if not bool(sel.any()):
            continue
        j = r["j"][sel]
        zj, zn = z[sel].gather(1, j[:, None])[:, 0], z[sel].gather(1, (j + 1)[:, None])[:, 0]
        assert bool(((zj <= zk[sel]) & (zk[sel] <= zn)).all()), (tag, tau)          # the bracket, in fp32
        # residual: the float64 transmittance at the kernel's own depth against L
        zq = zk.double()
        zq = torch.where(sel, zq, z64[:, 0])
        vis, _ = P.visibility(z, dists, ss, sd, b, zq)
        u = ulp32(zq)
        lo, _ = P.visibility(z, dists, ss, sd, b, zq - u)
        hi, _ = P.visibility(z, dists, ss, sd, b, zq + u)
        zterm = torch.maximum((lo - vis).abs(), (hi - vis).abs())
        kk = residual_k(r["F"], r["j"])
        bound = kk * U24 * torch.maximum(r["m_j"], torch.full_like(r["m_j"], r["L"]))
        res = (vis - r["L"]).abs()
        ratio = (res / (bound + zterm))[sel]
        worst = max(worst, float(ratio.max()))
        assert bool((ratio <= 1.0).all()), (tag, tau, float(ratio.max()))
        # depth, where the slope is above the floor
        width = (zn - zj).double()
        steep = r["slope"][sel] * width >= SLOPE_FLOOR * r["m_j"][sel]
        n_hit += int(sel.sum())
        n_floor += int((~steep).sum())
        derr = (zq[sel] - r["z"][sel]).abs()
        dbound = bound[sel] / r["slope"][sel].clamp(min=1e-300) + 2.0 * ulp32(r["z"][sel])
        assert bool((derr <= dbound)[steep].all()), (tag, tau, float((derr / dbound)[steep].max()))
        if bool(steep.any()):
            record_margin(f"{tag} tau={tau} depth vs float64 reference", float((derr / dbound)[steep].max()))
        # owner = num / den: two alphas (6 units each, absolute), two products and a sum put at most 8 units on num and 16 on
        # den; a share in [0, 1] moves by their sum over den, and the quotient rounds once more
        oerr = (got["owner"][k].cpu().double() - r["owner"])[sel].abs()
        obound = 24 * U24 / r["den"][sel].clamp(min=1e-30) + U24
        assert bool(((oerr <= obound) | (r["den"][sel] == 0)).all()), (tag, tau, float((oerr / obound).max()))
    record_margin(f"{tag} residual vs k 2^-24 max(L, m_j) + z term", worst)
    return worst, n_hit, n_floor, n_clear, n_all


def emulate_fp32(rays, z, sigma_s, sigma_d, blending, taus, scale):
    """the kernel's formulas in fp32 torch on the CPU (a sequential product in the place of the scan): dists, alpha_of,
    tfull_factor, the running minimum, the first crossing among s < S - 1, the smallest fp32 fraction t with
    m_j F_j(t dists_j) <= L by bisection over t's bit pattern, z_hit = min(z_j + t w, z_{j+1}) -> dict as hits_from_planes"""
    f32 = torch.float32
    N, S = z.shape
    nrm = (rays[:, 3] * rays[:, 3] + rays[:, 4] * rays[:, 4] + rays[:, 5] * rays[:, 5]).sqrt()[:, None]
    w = torch.cat([z[:, 1:] - z[:, :-1], torch.zeros(N, 1)], -1)
    ds = w * nrm * torch.tensor(scale, dtype=f32)

    def fac(sd, ss, b, d):
        a_d, a_s = 1.0 - torch.exp(-sd * d), 1.0 - torch.exp(-ss * d)
        return (1.0 - a_d * b) * (1.0 - a_s * (1.0 - b)) + torch.tensor(1e-10, dtype=f32)

    F = fac(sigma_d, sigma_s, blending, ds)
    T = torch.cumprod(torch.cat([torch.ones(N, 1), F], -1), -1)
    m = torch.cummin(T, -1).values
    out = dict(z=[], hit=[], owner=[])
    for tau in taus:
        L = torch.tensor(level(tau), dtype=f32)
        crossed = m[:, 1:] <= L
        crossed[:, S - 1] = False
        hit = crossed.any(-1)
        j = crossed.float().argmax(-1)
        g = lambda t: t.gather(1, j[:, None])[:, 0]
        mj, dj, sd, ss, b, zj, wj = g(m[:, :-1]), g(ds), g(sigma_d), g(sigma_s), g(blending), g(z), g(w)
        zn = g(torch.cat([z[:, 1:], z[:, -1:]], -1))
        lo = torch.zeros(N, dtype=torch.int64)                     # not crossed at lo
        hi = torch.full((N,), 0x3F800000, dtype=torch.int64)       # crossed at hi (t = 1: by the scan's word)
        for _ in range(31):
            mid = (lo + hi) // 2
            t = mid.to(torch.int32).view(f32)
            c = (mj * fac(sd, ss, b, t * dj) <= L) & (mid > lo)
            lo, hi = torch.where(c, lo, mid), torch.where(c, mid, hi)
        t = torch.where(mj <= L, torch.zeros(N), hi.to(torch.int32).view(f32))
        zh = torch.minimum(zj + t * wj, zn)
        a_d, a_s = 1.0 - torch.exp(-sd * dj), 1.0 - torch.exp(-ss * dj)
        num = a_d * b
        den = num + a_s * (1.0 - b)
        out["z"].append(torch.where(hit, zh, z[:, -1]))
        out["hit"].append(hit)
        out["owner"].append(torch.where(hit & (den != 0), num / torch.where(den != 0, den, torch.ones(N)), torch.zeros(N)))
    return {k: torch.stack(v) for k, v in out.items()}
