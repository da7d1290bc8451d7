"""Float64 reference, condition scales and seeded input regimes for the compositor (raw2outputs: k_composite /
composite_body, k_composite_bwd), shared by test_compositor_primitives_cpu.py and test_gpu_compositor_primitives.py.  No GPU.

Reference: oracle.rodynrf_oracle.raw2outputs on float64 tensors (test_oracle_golden.py pins it to the reference's own
fixtures) and torch autograd on it.  Inputs are fp32 numbers widened to float64, so both sides see the same values.

Condition scale: next to every output and every gradient the same quantity formed with each ADDED term replaced by its absolute
value (the sums over samples, the background terms 1 - acc, the assembly of the per-weight cotangents, the normaliser's
gwd - sum gwd w, the suffix sums of the transmittance gradients, the assembly of d/dalpha and d/dblending).  The gradients need
a written-out backward for that (`backward`), which test_compositor_primitives_cpu.py holds to autograd at 1e-12.  The
element-wise alpha = 1 - exp(-sigma dist) is NOT opened up: the regimes keep sigma dist >= ~1e-4 where it is not exactly 0, and
the 1e-4 max|ref| term of the bound carries its 2^-24 / alpha relative error.

Bound of every comparison (`tolerance`):  max|err| <= 1e-4 max|ref| + c(S) 2^-23 max(condition scale), with
c(S) = 6 S + S / 64 + 32 rounded operations on the longest path:
  * a transmittance is a product of up to S factors; each factor carries the rounding of sigma * dist (1), of expf (2 ulp: 2),
    of 1 - e (1), of + 1e-10 (1), and of its multiply into the scan (1): 6 S.  The order in which a scan associates the
    product does not change the count;
  * a per-ray sum is S / 64 sequential adds per lane and 6 butterfly levels; the suffix sums add one running total per tile:
    S / 64 + 6;
  * the per-sample arithmetic around them (weights, cotangent assembly, the normaliser's division, d/dalpha, d/dsigma) stays
    below 26 operations on any one path.

Regimes (`generate`): see REGIMES and the generator's comments.  dists are of order 1 / S so that the optical depth of a ray is
of order 1 at every S: the transmittance then changes by O(1) from tile to tile and a wrong carry is an O(1) error at S = 4096
as well.  The relu gate CAN be turned off with finite inputs (blending 1.5 on an opaque dynamic sample makes the product of
the full factors negative and acc_map_full > 1), so `gates` has such rays."""
import functools

import numpy as np
import torch

from oracle import rodynrf_oracle as O

ONAMES = ["rgb_map_full", "depth_map_full", "acc_map_full", "weights_full", "rgb_map_s", "depth_map_s", "acc_map_s",
          "weights_s", "rgb_map_d", "depth_map_d", "acc_map_d", "weights_d", "dynamicness_map"]
INAMES = ["rgb_s", "sigma_s", "rgb_d", "sigma_d", "dists", "blending", "z_vals", "rays"]
REGIMES = ["thin", "mixed", "wall", "double_wall", "empty_d", "empty_s", "empty_both", "blend_edges", "gates"]
RAY_TYPES = ("ndc", "contract", "world")
N_RAYS = 24                                    # 16 + 8: the grid-stride ray loop of composite_body is not at a multiple
SIZES = (1, 2, 63, 64, 65, 128, 129, 257)      # around the 64-sample tile: one lane, partial, full, full + 1, 2, 2 + 1, 4 + 1
EPS32 = 2.0 ** -23
SEED = 2                                       # of the seeds 0..5, 1, 2 and 4 keep every regime x size inside the 10 % redraw cap
RTOL = 1e-4                                    # _util.RTOL
GATE_MARGIN = 1e-3                             # `gates`: distance of every gated quantity from its kink
# the other regimes (colours in [0,1], blending in [0,1]: maps inside [0,1] up to rounding): c(S) 2^-23, the bound's own rounding
# term for a quantity of size 1 (gate_margin)
CONTRACT_DEPTH_ATOL = 256.0 * 2.0 ** -22       # test_golden_forward's absolute term of the contract depth maps
# the cotangent sets of the one-at-a-time backward test: each output alone, then the pairs the trainer's passes use
COT_SETS = [(i,) for i in range(13)] + [(4, 5), (9, 11)]


def c_ops(S):
    return 6 * S + S // 64 + 32


def gate_margin(regime, S):
    return GATE_MARGIN if regime == "gates" else c_ops(S) * EPS32


def tolerance(ref, cond, S, atol=0.0):
    """the bound of the module docstring for one tensor"""
    ref = torch.as_tensor(ref).double()
    cond = torch.as_tensor(cond).double()
    m = float(ref.abs().max()) if ref.numel() else 0.0
    cm = float(cond.abs().max()) if cond.numel() else 0.0
    return RTOL * m + c_ops(S) * EPS32 * cm + atol


def error_ratio(got, ref, cond, S, atol=0.0):
    got = torch.as_tensor(got).detach().cpu().double()
    ref = torch.as_tensor(ref).double()
    assert got.shape == ref.shape, f"shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    if ref.numel() == 0:
        return 0.0
    err = float((got - ref).abs().max())
    if not np.isfinite(err):
        return float("inf")
    return err / (tolerance(ref, cond, S, atol) + 1e-300)


def out_atol(k, ray_type):
    return CONTRACT_DEPTH_ATOL if (ray_type == "contract" and ONAMES[k].startswith("depth")) else 0.0


# ----------------------------------------------------------------------------------------------------------------------
# float64 forward pieces, the forward condition scales and the written-out backward
# ----------------------------------------------------------------------------------------------------------------------
def _excl_cumprod(p):
    one = torch.ones_like(p[:, :1])
    return torch.cumprod(torch.cat([one, p], -1), -1)[:, :-1]


def _suffix_excl(t):
    """sum of t over the samples AFTER each one, accumulated from the last sample towards the first"""
    sh = torch.cat([t[:, 1:], torch.zeros_like(t[:, :1])], -1)
    return sh.flip(-1).cumsum(-1).flip(-1)


def _pieces(x, white, ray_type):
    """every intermediate of raw2outputs, in the oracle's operation order"""
    q = dict(x)
    sd, ss, di, b = x["sigma_d"], x["sigma_s"], x["dists"], x["blending"]
    q["ed"], q["es"] = torch.exp(-sd * di), torch.exp(-ss * di)
    q["ad"], q["as"] = 1.0 - q["ed"], 1.0 - q["es"]
    q["pd"], q["ps"] = 1.0 - q["ad"] + 1e-10, 1.0 - q["as"] + 1e-10
    q["uu"], q["vv"] = 1.0 - q["ad"] * b, 1.0 - q["as"] * (1.0 - b)
    q["pf"] = q["uu"] * q["vv"] + 1e-10
    q["Td"], q["Ts"], q["Tf"] = _excl_cumprod(q["pd"]), _excl_cumprod(q["ps"]), _excl_cumprod(q["pf"])
    q["u"] = q["ad"] * q["Td"]
    q["U"] = q["u"].sum(-1, keepdim=True)
    q["Ue"] = q["U"] + 1e-10
    q["wd"] = q["u"] / q["Ue"]
    q["ws"] = q["as"] * q["Ts"]
    q["cfd"], q["cfs"] = q["ad"] * b, q["as"] * (1.0 - b)
    q["wf"] = (q["cfd"] + q["cfs"]) * q["Tf"]
    q["acc_d"], q["acc_s"], q["acc_f"] = q["wd"].sum(-1), q["ws"].sum(-1), q["wf"].sum(-1)
    q["rl_on"] = (1.0 - q["acc_f"]) > 0
    q["rl"] = torch.relu(1.0 - q["acc_f"])
    w = 1.0 if white else 0.0
    q["Rd"] = (q["wd"][..., None] * x["rgb_d"]).sum(-2) + w * (1.0 - q["acc_d"])[:, None]
    q["Rs"] = (q["ws"][..., None] * x["rgb_s"]).sum(-2) + w * (1.0 - q["acc_s"])[:, None]
    q["Rf"] = ((q["Tf"] * q["cfd"])[..., None] * x["rgb_d"] + (q["Tf"] * q["cfs"])[..., None] * x["rgb_s"]).sum(-2) \
        + w * q["rl"][:, None]
    if ray_type == "ndc":
        q["far"] = x["rays"][:, 2] + x["rays"][:, 5]
    elif ray_type == "contract":
        q["far"] = torch.full_like(q["acc_d"], 256.0)
    else:
        q["far"] = torch.zeros_like(q["acc_d"])
    return q


def forward_cond(x, white, ray_type):
    """the 13 condition scales of the outputs: each sum with its terms' absolute values"""
    q = _pieces(x, white, ray_type)
    w = 1.0 if white else 0.0
    far, z, b = q["far"].abs(), x["z_vals"].abs(), x["blending"].abs()
    wd, ws, wf = q["wd"].abs(), q["ws"].abs(), (q["cfd"].abs() + q["cfs"].abs()) * q["Tf"].abs()
    on = q["rl_on"].double()
    bg_d, bg_s, bg_f = 1.0 + wd.sum(-1), 1.0 + ws.sum(-1), on * (1.0 + wf.sum(-1))
    Rd = (wd[..., None] * x["rgb_d"].abs()).sum(-2) + w * bg_d[:, None]
    Rs = (ws[..., None] * x["rgb_s"].abs()).sum(-2) + w * bg_s[:, None]
    Rf = ((q["Tf"] * q["cfd"]).abs()[..., None] * x["rgb_d"].abs()
          + (q["Tf"] * q["cfs"]).abs()[..., None] * x["rgb_s"].abs()).sum(-2) + w * bg_f[:, None]
    return [Rf, (wf * z).sum(-1) + bg_f * far, wf.sum(-1), wf,
            Rs, (ws * z).sum(-1) + bg_s * far, ws.sum(-1), ws,
            Rd, (wd * z).sum(-1) + bg_d * far, wd.sum(-1), wd, (wf * b).sum(-1)]


def backward(x, cot, white, ray_type, absmode=False):
    """written-out backward of raw2outputs in float64.  cot: list of 13, None = no cotangent.  Returns the 8 input gradients
    (a zero tensor where no cotangent reaches).  absmode: every added term enters with its absolute value."""
    A = torch.abs if absmode else (lambda t: t)

    def add(*terms):
        s = A(terms[0])
        for t in terms[1:]:
            s = s + A(t)
        return s

    q = _pieces(x, white, ray_type)
    N, S = x["sigma_d"].shape
    w = 1.0 if white else 0.0
    zero_r, zero_s = torch.zeros(N, dtype=torch.float64), torch.zeros(N, S, dtype=torch.float64)
    G = [c if c is not None else (torch.zeros(N, 3, dtype=torch.float64) if k in (0, 4, 8) else
                                  (zero_s if k in (3, 7, 11) else zero_r)) for k, c in enumerate(cot)]
    gate = lambda R: ((R >= 0) & (R <= 1)).double()
    grf, grs, grd = G[0] * gate(q["Rf"]), G[4] * gate(q["Rs"]), G[8] * gate(q["Rd"])
    sgf, sgs, sgd = A(grf).sum(-1), A(grs).sum(-1), A(grd).sum(-1)
    Gdep_f, Gacc_f, Gdep_s, Gacc_s, Gdep_d, Gacc_d, Gdyn = G[1], G[2], G[5], G[6], G[9], G[10], G[12]
    far, z, b = q["far"], x["z_vals"], x["blending"]
    on = q["rl_on"].double()
    cd_, cs_ = x["rgb_d"], x["rgb_s"]
    dd = A(grd[:, None, :] * cd_).sum(-1)
    dsv = A(grs[:, None, :] * cs_).sum(-1)
    dfd = A(grf[:, None, :] * cd_).sum(-1)
    dfs = A(grf[:, None, :] * cs_).sum(-1)
    col = lambda v: v[:, None]
    gwd = add(G[11], dd, col(Gdep_d) * z, col(Gacc_d), col(-w * sgd), col(-Gdep_d * far))
    gws = add(G[7], dsv, col(Gdep_s) * z, col(Gacc_s), col(-w * sgs), col(-Gdep_s * far))
    gwf = add(G[3], col(Gdep_f) * z, col(Gdyn) * b, col(Gacc_f), col(on * (-w * sgf)), col(on * (-Gdep_f * far)))
    D1 = A(gwd * q["wd"]).sum(-1, keepdim=True)
    gu = add(gwd, -D1) / q["Ue"]
    sd_ = _suffix_excl(A(gu * q["u"]))
    ss_ = _suffix_excl(A(gws * q["ws"]))
    g_Tf = add(q["cfd"] * dfd, q["cfs"] * dfs, gwf * q["cfd"], gwf * q["cfs"])
    sf_ = _suffix_excl(A(q["Tf"] * g_Tf))
    g_pf = sf_ / q["pf"]
    g_cfd = q["Tf"] * add(dfd, gwf)
    g_cfs = q["Tf"] * add(dfs, gwf)
    g_ad = add(gu * q["Td"], -sd_ / q["pd"], g_cfd * b, -g_pf * b * q["vv"])
    g_as = add(gws * q["Ts"], -ss_ / q["ps"], g_cfs * (1.0 - b), -g_pf * q["uu"] * (1.0 - b))
    g_b = add(col(Gdyn) * q["wf"], g_cfd * q["ad"], -g_cfs * q["as"], -g_pf * q["ad"] * q["vv"], g_pf * q["uu"] * q["as"])
    di = x["dists"]
    g_sigma_d = g_ad * di * q["ed"]
    g_sigma_s = g_as * di * q["es"]
    g_dists = add(g_ad * x["sigma_d"] * q["ed"], g_as * x["sigma_s"] * q["es"])
    g_z = add(col(Gdep_d) * q["wd"], col(Gdep_s) * q["ws"], col(Gdep_f) * q["wf"])
    g_rgb_s = add(grs[:, None, :] * q["ws"][..., None], grf[:, None, :] * (q["Tf"] * q["cfs"])[..., None])
    g_rgb_d = add(grd[:, None, :] * q["wd"][..., None], grf[:, None, :] * (q["Tf"] * q["cfd"])[..., None])
    g_rays = torch.zeros(N, 6, dtype=torch.float64)
    if ray_type == "ndc":
        if absmode:
            gfar = Gdep_d.abs() * (1.0 + q["acc_d"].abs()) + Gdep_s.abs() * (1.0 + q["acc_s"].abs()) \
                + Gdep_f.abs() * on * (1.0 + q["acc_f"].abs())
        else:
            gfar = Gdep_d * (1.0 - q["acc_d"]) + Gdep_s * (1.0 - q["acc_s"]) + Gdep_f * q["rl"]
        g_rays[:, 2] = gfar
        g_rays[:, 5] = gfar
    return [g_rgb_s, g_sigma_s, g_rgb_d, g_sigma_d, g_dists, g_b, g_z, g_rays]


# ----------------------------------------------------------------------------------------------------------------------
# the reference proper: oracle + autograd, float64 or float32
# ----------------------------------------------------------------------------------------------------------------------
def widen(x32):
    return {k: v.double() for k, v in x32.items()}


def oracle_run(x32, white, ray_type, cot32=None, dtype=torch.float64):
    """oracle.raw2outputs and its autograd gradients in `dtype`.  cot32: None (forward only) or a list of 13 fp32 cotangents
    (None entries carry none).  Returns (outs[13], grads[8] or None); a gradient autograd does not give is None."""
    xs = {k: v.to(dtype).clone().requires_grad_(True) for k, v in x32.items()}
    outs = O.raw2outputs(*[xs[k] for k in INAMES], bool(white), ray_type)
    if cot32 is None:
        return [o.detach() for o in outs], None
    sel = [k for k in range(13) if cot32[k] is not None]
    g = torch.autograd.grad([outs[k] for k in sel], [xs[k] for k in INAMES], [cot32[k].to(dtype) for k in sel],
                            allow_unused=True)
    return [o.detach() for o in outs], list(g)


def cotangents(N, S, seed):
    """seeded random fp32 cotangents for all 13 outputs"""
    rng = np.random.RandomState(seed)
    shapes = [(N, 3), (N,), (N,), (N, S)] * 3 + [(N,)]
    return [torch.from_numpy(rng.standard_normal(s).astype(np.float32)) for s in shapes]


@functools.lru_cache(maxsize=None)
def reference(regime, N, S, white, ray_type, cot_set=None, seed=None):
    """Cached float64 reference of one case: dict with x (fp32 inputs), outs, fcond, and -- for cot_set (a tuple of output
    indices, or "all") -- cot (list of 13, None where unused), grads (None where autograd gives none) and gcond."""
    seed = SEED if seed is None else seed
    x32 = generate(regime, N, S, seed)
    r = dict(x=x32, S=S, N=N)
    x64 = widen(x32)
    cot = None
    if cot_set is not None:
        full = cotangents(N, S, 1000 + S)
        idx = range(13) if cot_set == "all" else cot_set
        cot = [full[k] if k in idx else None for k in range(13)]
    outs, grads = oracle_run(x32, white, ray_type, cot)
    r["outs"], r["fcond"] = outs, forward_cond(x64, white, ray_type)
    if cot is not None:
        c64 = [None if c is None else c.double() for c in cot]
        r["cot"], r["grads"] = cot, grads
        r["gcond"] = backward(x64, c64, white, ray_type, absmode=True)
    return r


# ----------------------------------------------------------------------------------------------------------------------
# regimes
# ----------------------------------------------------------------------------------------------------------------------
def wall_positions(n, S):
    """(dynamic wall, static wall) of ray n: successive rays put the dynamic wall at the first lane of a 64-sample tile, at the
    last lane of one, and in the last (partial) tile; the static wall sits elsewhere when S > 1"""
    ntile = (S + 63) // 64
    kind = n % 3
    if kind == 0:
        pd = 64 * ((n // 3) % ntile)
    elif kind == 1:
        pd = min(64 * ((n // 3) % ntile) + 63, S - 1)
    else:
        last0 = 64 * (ntile - 1)
        pd = last0 + (n // 3) % (S - last0)
    ps = (pd + 1 + (5 * n) % max(S - 1, 1)) % S if S > 1 else 0
    return pd, ps


def _base(rng, N, S, xmax=0.03):
    """thin rays: sigma dist in [0.1, 1] min(xmax, 1.5 / S) (total optical depth < 1), dists ~ 1 / S, blending in [0.2, 0.8],
    colours in [0, 1], increasing z_vals in (0, 1), NDC-like rays whose far plane rays[2] + rays[5] is near 1"""
    f32 = np.float32
    dists = (rng.uniform(0.5, 1.5, (N, S)) / S).astype(f32)
    scale = min(xmax, 1.5 / S)
    x = dict(
        rgb_s=rng.uniform(0, 1, (N, S, 3)).astype(f32),
        sigma_s=(rng.uniform(0.1, 1.0, (N, S)) * scale / dists).astype(f32),
        rgb_d=rng.uniform(0, 1, (N, S, 3)).astype(f32),
        sigma_d=(rng.uniform(0.1, 1.0, (N, S)) * scale / dists).astype(f32),
        dists=dists,
        blending=rng.uniform(0.2, 0.8, (N, S)).astype(f32),
        z_vals=(np.cumsum(rng.uniform(0.5, 1.5, (N, S)), -1) / (1.5 * S + 1)).astype(f32),
        rays=np.concatenate([rng.uniform(-1, 1, (N, 2)), -np.ones((N, 1)), rng.normal(0, 0.1, (N, 2)),
                             2.0 + rng.uniform(-0.1, 0.1, (N, 1))], -1).astype(f32),
    )
    return x


def _opaque(rng, dist, lo, hi):
    """a sigma with sigma * dist in [lo, hi] in fp32 too"""
    s = np.float32(rng.uniform(lo, hi) / dist)
    while np.float32(s * dist) <= np.float32(lo - 0.5):
        s = np.float32(s * 1.01)
    return s


def _draw(regime, N, S, rng):
    x = _base(rng, N, S, xmax=1.5 if regime == "gates" else (0.6 if regime == "blend_edges" else 0.03))
    f32 = np.float32
    if regime == "mixed":
        # sigma log-uniform over 1e-3 .. 1e3, ~70 % exactly zero; dists ~ 0.05 / S give a ray an optical depth of order 1
        x["dists"] = (rng.uniform(0.5, 1.5, (N, S)) * 0.05 / S).astype(f32)
        for k in ("sigma_s", "sigma_d"):
            s = 10.0 ** rng.uniform(-3, 3, (N, S))
            s[rng.uniform(size=(N, S)) < 0.7] = 0.0
            x[k] = s.astype(f32)
    elif regime == "wall":
        for n in range(N):
            pd, ps = wall_positions(n, S)
            x["sigma_d"][n, pd] = _opaque(rng, x["dists"][n, pd], 18.0, 60.0)
            if ps != pd:
                x["sigma_s"][n, ps] = _opaque(rng, x["dists"][n, ps], 18.0, 60.0)
    elif regime == "double_wall":
        for n in range(N):
            pd, ps = wall_positions(n, S)
            run = (2, 3, 5, 6)[n % 4]
            # the whole run fits (it may straddle a tile edge) and, where there is room, does not start the ray: the fourth
            # wall's own weight is then T 1e-30 with T <= 0.9995, clear of the 1e-30 line the GPU test draws
            pd = min(max(pd, 1), max(S - run, 0))
            for j in range(pd, min(pd + run, S)):
                x["sigma_d"][n, j] = _opaque(rng, x["dists"][n, j], 40.0, 80.0)
            for j in range(ps, min(ps + run, S)):     # never both fields opaque in one sample: acc_map_full would be 1 +- ulp
                if not pd <= j < pd + run:
                    x["sigma_s"][n, j] = _opaque(rng, x["dists"][n, j], 40.0, 80.0)
    elif regime == "empty_d":
        x["sigma_d"][:] = 0
    elif regime == "empty_s":
        x["sigma_s"][:] = 0
    elif regime == "empty_both":
        x["sigma_d"][:] = 0
        x["sigma_s"][:] = 0
    elif regime == "blend_edges":
        j = np.arange(S)
        for n in range(N):
            kind = n % 4
            if kind == 0:
                x["blending"][n] = 0
            elif kind == 1:
                x["blending"][n] = 1
            else:
                x["blending"][n] = ((j + n // 4) % 2).astype(f32)
            pd, _ = wall_positions(n, S)
            if kind == 3 and pd >= 1:
                # an opaque dynamic sample with blending 1: its full factor is 1e-10 exactly and d/dblending there is a
                # quotient of two numbers of that size.  Such a ray has acc_map_full = 1 +- rounding, on the relu's kink; the
                # sample before it (both alphas 0.63, blending 0.5: the ONE sample of these rays off the edges) adds
                # T alpha_d alpha_s b (1 - b) ~ 0.04 to acc_map_full and so holds the relu gate robustly closed
                x["sigma_d"][n, pd - 1] = f32(1.0 / x["dists"][n, pd - 1])
                x["sigma_s"][n, pd - 1] = f32(1.0 / x["dists"][n, pd - 1])
                x["blending"][n, pd - 1] = 0.5
                x["sigma_d"][n, pd] = _opaque(rng, x["dists"][n, pd], 40.0, 80.0)
                x["blending"][n, pd] = 1.0
    elif regime == "gates":
        x["rgb_s"] = rng.uniform(-0.5, 1.8, (N, S, 3)).astype(f32)
        x["rgb_d"] = rng.uniform(-0.5, 1.8, (N, S, 3)).astype(f32)
        for n in range(N):
            if n % 6 == 0:
                x["blending"][n] = rng.uniform(-0.5, 1.5, S).astype(f32)
            elif n % 6 == 3:   # acc_map_full > 1: no static density, an opaque-ish last dynamic sample with blending 1.5
                x["sigma_s"][n] = 0
                x["sigma_d"][n, S - 1] = f32(rng.uniform(2.0, 3.0) / x["dists"][n, S - 1])
                x["blending"][n, S - 1] = 1.5
    return x


def gate_margins(x32):
    """per ray: the smallest distance of a pre-clamp colour map from 0 and from 1, and of 1 - acc_map_full from 0, over both
    background settings, with the EXACT cases (a map that is exactly 0.0 or 1.0 in float64) left out.  float64, [N]."""
    x = widen(x32)
    m = torch.full((x["sigma_d"].shape[0],), float("inf"), dtype=torch.float64)
    for white in (False, True):
        q = _pieces(x, white, "world")
        for R in (q["Rf"], q["Rs"], q["Rd"]):
            for edge in (0.0, 1.0):
                d = (R - edge).abs()
                d = torch.where(d == 0, torch.full_like(d, float("inf")), d)
                m = torch.minimum(m, d.min(-1).values)
        d = (1.0 - q["acc_f"]).abs()
        m = torch.minimum(m, torch.where(d == 0, torch.full_like(d, float("inf")), d))
    return m


REDRAWS = {}    # (regime, N, S, seed) -> number of rays that were redrawn


@functools.lru_cache(maxsize=None)
def _generate(regime, N, S, seed):
    assert regime in REGIMES
    rng = np.random.RandomState((REGIMES.index(regime) * 7919 + S * 31 + seed) % (2 ** 31))
    x = _draw(regime, N, S, rng)
    redrawn = 0
    for attempt in range(1, 9):
        t = {k: torch.from_numpy(v) for k, v in x.items()}
        bad = (gate_margins(t) < gate_margin(regime, S)).numpy()
        if not bad.any():
            break
        redrawn += int(bad.sum())
        y = _draw(regime, N, S, np.random.RandomState((REGIMES.index(regime) * 7919 + S * 31 + seed + 104729 * attempt)
                                                      % (2 ** 31)))
        for k in x:
            x[k][bad] = y[k][bad]
    else:
        raise AssertionError(f"{regime} S={S}: gate margins not reached")
    # the reference's own rounding must not decide a gate, and the inputs must not be mostly redraws
    assert redrawn <= N // 10, f"{regime} S={S}: {redrawn} of {N} rays redrawn (cap 10 %)"
    REDRAWS[(regime, N, S, seed)] = redrawn
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in x.items()}


def generate(regime, N, S, seed=None):
    """the eight fp32 inputs of raw2outputs for N rays x S samples, as a dict by INAMES (fresh tensors: callers may move them)"""
    return {k: v.clone() for k, v in _generate(regime, N, S, SEED if seed is None else seed).items()}


def expected_none(cot_set, ray_type):
    """which inputs get NO gradient from a cotangent set, by the data flow of raw2outputs (renderer.py:173-315): the test holds
    autograd to this table as well"""
    s = set(range(13)) if cot_set == "all" else set(cot_set)
    depth = bool(s & {1, 5, 9})
    return [not (s & {0, 4}),                                   # rgb_s
            not (s & {0, 1, 2, 3, 4, 5, 6, 7, 12}),             # sigma_s
            not (s & {0, 8}),                                   # rgb_d
            not (s & {0, 1, 2, 3, 8, 9, 10, 11, 12}),           # sigma_d
            False,                                              # dists
            not (s & {0, 1, 2, 3, 12}),                         # blending
            not depth,                                          # z_vals
            not (depth and ray_type == "ndc")]                  # rays
