"""Float64 reference, condition scales and seeded input regimes for the per-field ray scan (forward: k_ray_scan 32 wide,
k_static_scan 64 wide; backward: k_ray_scan_bwd, k_static_density_bwd), shared by test_scan_primitives_cpu.py and
test_gpu_scan_primitives.py.  No GPU.  One level below tests/_comp_prim.py, whose regimes, dists of order 1 / S and bound it reuses.

Forward (float32 inputs widened to float64):  dz_j = z_{j+1} - z_j (0 behind the last sample), ds = dz |d| scale (|d| = 1 for world
rays), alpha = 1 - exp(-sigma ds), p = 1 - alpha + 1e-10, T = exclusive product of p, w = alpha T.  On the backward side
sigma = valid ? act(raw) : 0 with act = softplus(raw + shift) (beta 1, threshold 20) or relu(raw).

Backward: torch autograd over that forward (`reference`), plus a written-out backward (`backward`) that supplies the condition
scales -- every ADDED term replaced by its absolute value: the suffix sums of gw w, gw T - suffix / p, the assembly of g_sigma
and g_ds, the two-sided accumulation of g_z and the per-ray sum g_nrm.  test_scan_primitives_cpu.py holds the two to 1e-12.

What is returned is exactly what each kernel writes: width 32 `gsig`, the total d(sigma) = g_sigma + g_alpha ds (1 - alpha) of
EVERY sample; width 64 `gf` = gsig act'(raw) at valid samples and 0 at invalid ones.  At an invalid sample the reference follows
scan_sample / scan_bwd_step: its sigma is 0, but it still has a ds, still takes part in g_z and g_nrm (through the caller's
g_dists: g_alpha sigma (1 - alpha) is 0 there) and still passes the caller's g_sigma through to gsig.  Those samples are compared
like every other one; nothing is masked out.

Bound of every comparison:  max|err| <= 1e-4 max|ref| + c 2^-23 max(condition scale), with c = c_ops(S, width, softplus) =
_comp_prim.c_ops(S) = 6 S + S / 64 + 32 adjusted where this path has other rounded operations than the compositor's:
  * + 5 S: the compositor was handed dists; here every factor's ds is formed from z: the subtraction z_{j+1} - z_j (1), the
    product with |d| (1) and with the scale (1), and |d| = sqrt(x x + y y + z z) itself is off by up to 2 ulp (3 products and 2
    sums under the root: 2.5 ulp of the sum, halved by the root, plus the root's own half) in every factor of the ray (2);
  * + 5 S on the backward side with softplus: sigma = log1p(exp(raw + shift)): the sum (1), expf (2), log1pf (2) per factor;
    relu is exact.  (act' = sigmoid(raw + shift) is per-sample arithmetic, inside the 32.);
  * + S / 32 - S / 64 for width 32: a running total (carry, suffix sum, per-lane g_nrm) per 32-sample tile, not per 64.
Neither number was tuned against the kernels.

Regimes: `thin`, `mixed`, `empty` are _comp_prim's draws (its dynamic field's sigma, its dists -- which z_vals here are built to
reproduce: z_j = sum_{i<j} dists_i / (|d| scale) -- and its rays).  `wall` and `double_wall` are its thin draw with its opaque
samples (_opaque: sigma dist in 18 .. 60, runs of 2, 3, 5, 6 at 40 .. 80) at positions of this file's own (`wall_position`):
_comp_prim.wall_positions knows the 64-sample tiles of the compositor only and may choose the last sample, which has ds = 0 here and
cannot be opaque.  Successive rays put the wall at sample 0 and at 32 k - 1 and 32 k for every k, the last sample left out: both
sides of every 32-sample edge, the 64-sample edges among them (test_scan_primitives_cpu.py asserts it; at S = 4096 that takes the
255 rays of `edge_sweep_rays`, the N = 3 case of that size holds three of the positions).  Two more:
  * `invalid`: the `wall` regime with rays that have no valid sample (n % 3 == 0), rays valid in one 32-sample tile only (1) and rays
    whose valid flag alternates (2);
  * `act_edges`: raw at 10^U(log10 m - 0.1, 0) on either side of the activation's kink (relu: 0; softplus: 20 - shift), m =
    c 2^-23 being the bound's own distance; a sample closer than m to the kink is redrawn, and at most 10 % of a case's samples may
    be (REDRAWS).  The expected share is 0.1 / (0.1 - log10 m): 2 % at S = 1 to 4.5 % at S = 4096 with softplus; it depends on S
    through m and hardly on the seed, and a larger operation count moves it towards the cap only slowly (m = 0.03: 6 %)."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import _comp_prim as P

REGIMES = ["thin", "mixed", "wall", "double_wall", "empty", "invalid", "act_edges"]
_COMP_DRAW = {"thin": "thin", "mixed": "mixed", "wall": "thin", "double_wall": "thin", "empty": "empty_d", "invalid": "thin",
              "act_edges": "thin"}
RAY_TYPES = P.RAY_TYPES
ACTS = ("relu", "softplus")
N_RAYS = 35                                     # width 32: two full 16-ray workgroups + 3 rays (one half-wave idle); width 64: 8 x 4 + 3
SIZES = (1, 2, 31, 32, 33, 63, 64, 65, 129, 257)
S_MAX = 4096
SHIFT = -10.0                                   # the reference's density_shift
SEED = 0                                        # the redraw share of act_edges is set by S, not by the seed (module docstring)
COT_SETS = [("w",), ("s",), ("d",), ("w", "s"), ("w", "d"), ("s", "d"), ("w", "s", "d")]
EPS32, RTOL = P.EPS32, P.RTOL


def c_ops(S, width=64, softplus=False):
    return P.c_ops(S) + 5 * S + (5 * S if softplus else 0) + (S // 32 - S // 64 if width == 32 else 0)


def tolerance(ref, cond, c):
    m = float(ref.abs().max()) if ref.numel() else 0.0
    cm = float(cond.abs().max()) if cond.numel() else 0.0
    return RTOL * m + c * EPS32 * cm


def error_ratio(got, ref, cond, c):
    got = torch.as_tensor(got).detach().cpu().double()
    assert got.shape == ref.shape, f"shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    if ref.numel() == 0:
        return 0.0
    err = float((got - ref).abs().max())
    if not np.isfinite(err):
        return float("inf")
    return err / (tolerance(ref, cond, c) + 1e-300)


# ----------------------------------------------------------------------------------------------------------------------
# float64 forward, written-out backward, autograd
# ----------------------------------------------------------------------------------------------------------------------
def density_act(raw, act, shift=SHIFT):
    return F.softplus(raw + shift, beta=1.0, threshold=20.0) if act == "softplus" else torch.relu(raw)


def _geometry(rays, z, ray_type, scale):
    d = rays[:, 3:6]
    nrm = torch.ones_like(z[:, :1]) if ray_type == "world" else d.norm(dim=-1, keepdim=True)
    dz = torch.cat([z[:, 1:] - z[:, :-1], torch.zeros_like(z[:, :1])], -1)
    return d, nrm, dz, dz * nrm * scale


def forward(rays, z, sigma, ray_type, scale):
    """dict of every intermediate: dz, nrm, ds, e = exp(-sigma ds), alpha, p, T, w"""
    d, nrm, dz, ds = _geometry(rays, z, ray_type, scale)
    e = torch.exp(-sigma * ds)
    alpha = 1.0 - e
    p = 1.0 - alpha + 1e-10
    T = P._excl_cumprod(p)
    return dict(d=d, nrm=nrm, dz=dz, ds=ds, e=e, alpha=alpha, p=p, T=T, w=alpha * T)


def backward(rays, z, valid, raw, act, ray_type, scale, gw=None, gs=None, gd=None, absmode=False, shift=SHIFT):
    """written-out backward in float64; None cotangents carry nothing.  Returns dict(gsig, gf, g_z, g_rays).  absmode: every added
    term enters with its absolute value (the condition scales)."""
    A = torch.abs if absmode else (lambda t: t)
    zero = torch.zeros_like(z)
    gw, gs, gd = (zero if g is None else g for g in (gw, gs, gd))
    on = valid.bool()
    sigma = torch.where(on, density_act(raw, act, shift), zero)
    q = forward(rays, z, sigma, ray_type, scale)
    suffix = P._suffix_excl(A(gw * q["w"]))
    g_alpha = A(gw * q["T"]) + A(-suffix / q["p"])
    one_m = q["e"]                                                    # 1 - alpha, without float64's own cancellation behind a wall
    gsig = A(gs) + A(g_alpha * q["ds"] * one_m)
    g_ds = A(gd) + A(g_alpha * sigma * one_m)
    k = g_ds * q["nrm"] * scale
    k = torch.cat([k[:, :-1], zero[:, :1]], -1)                       # the last sample has no interval
    g_z = A(-k) + A(torch.cat([zero[:, :1], k[:, :-1]], -1))
    g_rays = torch.zeros_like(rays)
    if ray_type != "world":
        g_nrm = A(g_ds * q["dz"] * scale).sum(-1, keepdim=True)
        g_rays[:, 3:6] = A(g_nrm * q["d"] / q["nrm"])
    if act == "softplus":
        dact = torch.sigmoid(raw + shift)
        dact = torch.where(raw + shift > 20.0, torch.ones_like(dact), dact)
    else:
        dact = (raw > 0).double()
    return dict(gsig=gsig, gf=torch.where(on, gsig * dact, zero), g_z=g_z, g_rays=g_rays)


def autograd_backward(rays, z, valid, raw, act, ray_type, scale, gw=None, gs=None, gd=None, shift=SHIFT):
    """the same four results from torch autograd over `forward`"""
    rays = rays.clone().requires_grad_(True)
    z = z.clone().requires_grad_(True)
    raw = raw.clone().requires_grad_(True)
    on = valid.bool()
    a = density_act(raw, act, shift)
    sigma = torch.where(on, a, torch.zeros_like(a)).detach().requires_grad_(True)
    q = forward(rays, z, sigma, ray_type, scale)
    L = (sigma * 0).sum() + (z * 0).sum() + (rays * 0).sum()
    for g, t in ((gw, q["w"]), (gs, sigma), (gd, q["ds"])):
        if g is not None:
            L = L + (g * t).sum()
    gsig, g_z, g_rays = torch.autograd.grad(L, [sigma, z, rays])
    gf, = torch.autograd.grad(a, raw, gsig * on.double())
    return dict(gsig=gsig, gf=gf, g_z=g_z, g_rays=g_rays)


# ----------------------------------------------------------------------------------------------------------------------
# regimes
# ----------------------------------------------------------------------------------------------------------------------
REDRAWS = {}    # (regime, N, S, act, seed) -> share of the samples that were redrawn


def _rng(regime, S, seed, k=0):
    return np.random.RandomState((REGIMES.index(regime) * 7919 + S * 31 + seed + 104729 * k) % (2 ** 31))


def _softplus_inv(s):
    s = np.asarray(s, np.float64)
    return np.where(s > 20.0, s, np.log(np.expm1(np.minimum(s, 20.0)) + 1e-300))


def wall_candidates(S):
    """sample 0, then both sides of every 32-sample edge, without the last sample (ds = 0 behind it)"""
    c = [0] + [p for k in range(1, (S - 1) // 32 + 1) for p in (32 * k - 1, 32 * k)]
    return [p for p in c if p < S - 1] or [0]


def wall_position(n, S):
    c = wall_candidates(S)
    return c[n % len(c)]


def edge_sweep_rays(S):
    """the number of rays after which `wall_position` has been everywhere"""
    return len(wall_candidates(S))


@functools.lru_cache(maxsize=None)
def _generate(regime, N, S, act, ray_type, scale, seed):
    assert regime in REGIMES
    f32 = np.float32
    rng = _rng(regime, S, seed)
    x = P._draw(_COMP_DRAW[regime], N, S, rng)
    rays, dists, sigma = x["rays"], x["dists"].astype(np.float64), x["sigma_d"].astype(np.float64)
    nrm = np.ones(N) if ray_type == "world" else np.linalg.norm(rays[:, 3:6].astype(np.float64), axis=-1)
    # z whose intervals reproduce the draw's dists: ds = dz |d| scale ~ dists, of order 1 / S
    step = dists / (nrm[:, None] * scale)
    z = (rng.uniform(0.0, 0.5, (N, 1)) * step[:, :1] + np.concatenate([np.zeros((N, 1)), np.cumsum(step, -1)[:, :-1]], -1)).astype(f32)
    if regime in ("wall", "double_wall", "invalid"):
        sig32 = x["sigma_d"]
        for n in range(N):
            pd = wall_position(n, S)
            if regime == "double_wall":   # the whole run in front of the last sample, on both sides of its edge where it starts on one
                run = (2, 3, 5, 6)[n % 4]
                for j in range(min(pd, max(S - 1 - run, 0)), min(pd + run, S - 1)):
                    sig32[n, j] = P._opaque(rng, x["dists"][n, j], 40.0, 80.0)
            else:
                sig32[n, pd] = P._opaque(rng, x["dists"][n, pd], 18.0, 60.0)
        sigma = sig32.astype(np.float64)
    valid = np.ones((N, S), np.uint8)
    if regime == "invalid":
        j = np.arange(S)
        ntile = (S + 31) // 32
        for n in range(N):
            if n % 3 == 0:
                valid[n] = 0
            elif n % 3 == 1:
                valid[n] = (j // 32 == (n // 3) % ntile)
            else:
                valid[n] = (j + n // 3) % 2
    # raw with act(raw) ~ sigma: relu's zeros sit at negative raws, softplus's at raw + shift = -30 (sigma 9e-14)
    if act == "relu":
        raw = np.where(sigma > 0, sigma, -rng.uniform(0.1, 2.0, (N, S)))
    else:
        raw = np.where(sigma > 0, _softplus_inv(np.maximum(sigma, 1e-13)), -30.0) - SHIFT
    share = 0.0
    if regime == "act_edges":
        kink = 0.0 if act == "relu" else 20.0 - SHIFT
        m = c_ops(S, 32, act == "softplus") * EPS32

        def draw(r):
            return kink + r.choice([-1.0, 1.0], (N, S)) * 10.0 ** r.uniform(np.log10(m) - 0.1, 0.0, (N, S))

        raw = draw(rng).astype(f32)
        redrawn = 0
        for k in range(1, 9):
            bad = np.abs(raw.astype(np.float64) - kink) < m
            if not bad.any():
                break
            redrawn += int(bad.sum())
            raw[bad] = draw(_rng(regime, S, seed, k)).astype(f32)[bad]
        else:
            raise AssertionError(f"act_edges S={S} {act}: margin not reached")
        share = redrawn / float(N * S)
        assert share <= 0.10, f"act_edges S={S} {act}: {share:.3f} of the samples redrawn (cap 10 %)"
    REDRAWS[(regime, N, S, act, seed)] = share
    out = dict(rays=rays.astype(f32), z=z, raw=np.asarray(raw, f32), valid=valid)
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in out.items()}


def generate(regime, N, S, act="relu", ray_type="ndc", scale=25.0, seed=None):
    """fp32 rays [N,6], z [N,S], raw [N,S], valid [N,S] uint8, and sigma [N,S] = fp32(valid ? act(raw) : 0), the forward entry's input"""
    x = {k: v.clone() for k, v in _generate(regime, N, S, act, ray_type, float(scale), SEED if seed is None else seed).items()}
    s = density_act(x["raw"].double(), act)
    x["sigma"] = torch.where(x["valid"].bool(), s, torch.zeros_like(s)).float()
    return x


def cotangents(N, S, seed):
    rng = np.random.RandomState(seed)
    return {k: torch.from_numpy(rng.standard_normal((N, S)).astype(np.float32)) for k in ("w", "s", "d")}


def reference_of(x, S, act, ray_type, scale, cot_set=None):
    """float64 reference of the inputs x (as `generate` returns them): see `reference`"""
    N = x["z"].shape[0]
    r = dict(x=x, N=N, S=S)
    q = forward(x["rays"].double(), x["z"].double(), x["sigma"].double(), ray_type, scale)
    r["fwd"] = dict(w=q["w"], ds=q["ds"], wcond=q["w"].abs(), alpha=q["alpha"])
    if cot_set is not None:
        full = cotangents(N, S, 1000 + S)
        cot = {k: (full[k] if k in cot_set else None) for k in ("w", "s", "d")}
        c64 = {k: (None if v is None else v.double()) for k, v in cot.items()}
        args = (x["rays"].double(), x["z"].double(), x["valid"], x["raw"].double(), act, ray_type, scale)
        r["cot"] = cot
        r["grads"] = autograd_backward(*args, gw=c64["w"], gs=c64["s"], gd=c64["d"])
        r["gcond"] = backward(*args, gw=c64["w"], gs=c64["s"], gd=c64["d"], absmode=True)
    return r


@functools.lru_cache(maxsize=None)
def reference(regime, N, S, act="relu", ray_type="ndc", scale=25.0, cot_set=None, seed=None):
    """Cached float64 reference of one case: x (fp32 inputs), fwd (the forward on x["sigma"]: w, ds and their condition scales) and,
    for cot_set (a tuple out of "w", "s", "d"), cot (fp32, None where unused), grads and gcond (dicts gsig, gf, g_z, g_rays)"""
    return reference_of(generate(regime, N, S, act, ray_type, scale, seed), S, act, ray_type, scale, cot_set)


def opaque_sigma(x, n, k, ray_type, scale, depth=25.0):
    """an fp32 sigma whose fp32 product with the kernel's ds at sample k of ray n is at least `depth` - 1"""
    q = forward(x["rays"].double(), x["z"].double(), x["sigma"].double() * 0, ray_type, scale)
    ds = float(q["ds"][n, k])
    assert ds > 0
    return float(np.float32(depth / ds))


# walls of the five rays of `walls_case` at S = 257: on an edge of both tile widths, in the first tile, in the last tile, in four
# consecutive 64-sample tiles and in four consecutive 32-sample tiles (transmittance behind them 1e-40)
WALLS = ((31, 32, 63, 64), (3,), (255,), (10, 70, 130, 190), (10, 40, 70, 100))
WALLS_S = 257


def walls_case(act="relu", ray_type="ndc", scale=25.0):
    """the `thin` draw at S = 257 with the opaque samples of WALLS (sigma ds ~ 25: alpha is 1.0 and p is 1e-10 in fp32)"""
    x = generate("thin", len(WALLS), WALLS_S, act, ray_type, scale)
    for n, pos in enumerate(WALLS):
        for k in pos:
            s = opaque_sigma(x, n, k, ray_type, scale)
            x["raw"][n, k] = s if act == "relu" else s - SHIFT
    s = density_act(x["raw"].double(), act)
    x["sigma"] = s.float()
    return x
