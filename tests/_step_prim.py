"""Float64 references, seeded generators and error bounds for the kernels that run once per iteration NEXT to the ray path:
csrc/rdrf_optim.hip (k_adam, k_upsample, k_dense_l1), csrc/rdrf_loss.hip (k_loss_*, k_frame_depth_loss) and csrc/rdrf_misc.hip
(k_distloss*, k_tv_*, k_rows_scatter_add).  Shared by test_step_primitives_cpu.py (keeps these references honest against
torch / the oracle / tests/golden/tv.npz in float64, and shows that a float32 torch evaluation meets every bound) and
test_gpu_step_primitives.py (holds the kernels to them).

Every reference takes the SAME float32 inputs the kernel gets, widens them to float64 and returns, next to the result, a
CONDITION SCALE per output: the sum of the absolute values of the terms the output adds up.  Every bound is

    |got - ref| <= k * 2^-24 * condition scale  (+ half an ulp of the stored result where the kernel rounds into memory)

with k counted from the kernel's own operations (one unit roundoff 2^-24 per rounded operation on the path of a term, plus the
depth of the summation the term goes through).  The counts are the k_* functions below, each with its derivation; none was tuned
against the kernels.  Where the condition scale is 0 the bound is 0: the result must be exact."""
import math

import numpy as np
import torch

U = 2.0 ** -24
F32 = np.float32


def f64(x):
    return np.asarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x, dtype=np.float64)


def half_ulp(x):
    """half the float32 spacing at |x| (what one rounding of a stored value may add)"""
    return 0.5 * np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(F32)).astype(np.float64)


def error_ratio(got, ref, cond, k, extra=0.0):
    """max over the elements of |got - ref| / (k 2^-24 cond + extra); an element whose bound is 0 must be exact (ratio 0 or inf)"""
    got, ref, cond = f64(got), f64(ref), np.broadcast_to(f64(cond), np.shape(f64(ref)))
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if not np.isfinite(got).all():
        return math.inf
    err = np.abs(got - ref)
    tol = k * U * cond + extra
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0


def rng(*key):
    return np.random.default_rng([17, *[int(k) for k in key]])


# ----------------------------------------------------------------------------------------------------------------------------
# Adam (k_adam).  The kernel receives lr, betas, eps, grad_scale as float32 and the two bias corrections as float32 roundings of
# their float64 values: the reference uses exactly those float32 constants, widened, and float64 arithmetic on them.
#   m' = m + (gr - m)(1 - b1),  gr = g gs:   4 roundings (gr, the difference, its product, the sum)         -> K_ADAM_M = 4
#      on the terms |m| + (1 - b1)(|gr| + |m|)
#   v' = v b2 + (1 - b2) gr gr:  gr twice (2), two products (2), v b2 (1), the sum (1); all terms >= 0      -> K_ADAM_V = 6
#   update = -step_size m' / (sqrt(v') isb + eps): sqrt(v') carries K_ADAM_V / 2 + 1, isb is a rounded constant (1), its product
#      and the sum (2): 7 on the denominator; the quotient (1), step_size = lr * inv_bc1 (a rounded constant and a product: 2) and
#      the last product (1): 11 on |m'|, plus the error of m' itself (K_ADAM_M on its terms)                 -> K_ADAM_UPD = 11
#      on step_size / denom * (|m'| + terms of m');  p' = p - update is stored: + half an ulp of p'.
# ----------------------------------------------------------------------------------------------------------------------------
K_ADAM_M, K_ADAM_V, K_ADAM_UPD = 4, 6, 11
ADAM_GRID = 2048 * 256 * 4            # elements one pass of the capped grid covers: beyond it the grid-stride loop runs
ADAM_SIZES = (4, 1028, ADAM_GRID + 1028)
ADAM_HYPER = dict(lr0=0.02, lr1=1e-3, beta1=0.9, beta2=0.99, eps=1e-8)


def adam_ref(p, g, m, v, split, step, grad_scale, lr0, lr1, beta1, beta2, eps, f32_consts=True):
    """one step in float64 from float32 p, g, m, v -> dict(p, m, v, upd, cond_m, cond_v, cond_upd).  f32_consts: round the
    hyper-parameters as the C ABI does (False: plain float64 constants, the form torch.optim.Adam in float64 computes)"""
    c = (lambda x: float(F32(x))) if f32_consts else float
    p, g, m, v = f64(p), f64(g), f64(m), f64(v)
    b1, b2, gs, ep = c(beta1), c(beta2), c(grad_scale), c(eps)
    one_b1, one_b2 = c(1.0 - b1), c(1.0 - b2)          # (1.0f - beta: exact in float32 for beta in [0.5, 1])
    inv_bc1, isb = c(1.0 / (1.0 - b1 ** step)), c(1.0 / math.sqrt(1.0 - b2 ** step))
    lr = np.where(np.arange(p.size) < split, c(lr0), c(lr1))
    gr = g * gs
    m1 = m + (gr - m) * one_b1
    v1 = v * b2 + one_b2 * gr * gr
    denom = np.sqrt(v1) * isb + ep
    upd = -(lr * inv_bc1) * (m1 / denom)
    cond_m = np.abs(m) + one_b1 * (np.abs(gr) + np.abs(m))
    return dict(p=p + upd, m=m1, v=v1, upd=upd, cond_m=cond_m, cond_v=v1,
                cond_upd=(lr * inv_bc1) / denom * (np.abs(m1) + cond_m))


def adam_inputs(n, seed, state="zero"):
    """float32 p, g, m, v.  g spans 1e-6 .. 1e6 in magnitude; elements [8, 16) and the last four (the last two at n = 4, so
    that both learning rates still meet non-zero elements there) are EXACT zeros of g, m and v (their update must be exactly 0).  state "zero": m = v = 0 (a first step); "warm": seeded non-zero moments."""
    r = rng(1, n, seed)
    p = r.standard_normal(n).astype(F32)
    g = (r.standard_normal(n) * 10.0 ** r.uniform(-6, 6, n)).astype(F32)
    m, v = np.zeros(n, F32), np.zeros(n, F32)
    if state == "warm":
        gp = (r.standard_normal(n) * 10.0 ** r.uniform(-6, 6, n)).astype(F32)
        m, v = (0.3 * gp).astype(F32), (0.05 * gp.astype(np.float64) ** 2).astype(F32)
    z = np.r_[np.arange(8, 16)[np.arange(8, 16) < n], np.arange(n - min(4, n // 2), n)]
    g[z], m[z], v[z] = 0, 0, 0
    return p, g, m, v, z


def adam_splits(n):
    return sorted({0, 4, n - 4, n})


# ----------------------------------------------------------------------------------------------------------------------------
# Loss terms (k_loss_fwd / k_loss_stats / k_loss_finish / k_loss_bwd)
#   value_k = coef_k [* coef_dev] * sum_rows w sum_cols rho(x + ysign y) / Z,  Z = rows cols | sum_ranks(sum w) / world + 1e-8
# Per element: r (1), rho (1), the weight (1) = 3.  Summation of 128 x 256 threads: the serial grid-stride part of a thread,
# T = ceil(total / 32768) adds, six wave steps, two levels of the four-way block sum, the serial sum over the 128 partials (127):
# T + 135.  The weight sum takes the same road (T + 135) and enters through Z with two more (the division by world, + 1e-8).  The
# finish: the coefficient product, the division by Z, the product with the sum (3), and the rank statistics added in float32 (1).
#   k_loss = 3 + 2 (T + 135) + 2 + 4          on  |coef| / Z * sum |w| |rho|
#   k_grad = (T + 135) + 2 + 3 + 4            on  |gradient|   (Z and the coefficient, then g_loss * scale, r, and two products)
# ----------------------------------------------------------------------------------------------------------------------------
LOSS_BLOCK_ELEMS = 128 * 256
LOSS_SHAPES = ((1, 1), (7, 1), (5, 3), (255, 1), (32767, 1), (32768, 1), (32769, 1), (10923, 3), (777, 111))
LOSS_KINDS = ("square", "abs", "identity")


def k_loss(total):
    return 3 + 2 * (math.ceil(total / LOSS_BLOCK_ELEMS) + 135) + 2 + 4


def k_loss_grad(total):
    return math.ceil(total / LOSS_BLOCK_ELEMS) + 135 + 2 + 3 + 4


def _rho(kind, r):
    return r * r if kind == "square" else (np.abs(r) if kind == "abs" else r)


def _drho(kind, r):
    return 2.0 * r if kind == "square" else (np.sign(r) if kind == "abs" else np.ones_like(r))


def loss_stats(kind, x, y, ysign, w):
    """(sum_rows w sum_cols rho, sum_rows w, sum |w| |rho|) in float64; x [rows, cols]"""
    x = f64(x)
    r = x + (0.0 if y is None else ysign * f64(y))
    wv = np.ones(x.shape[0]) if w is None else f64(w)
    t = wv[:, None] * _rho(kind, r)
    return float(t.sum()), float(wv.sum()), float(np.abs(t).sum())


def loss_ref(kind, norm, x, y=None, ysign=-1.0, w=None, coef=1.0, global_ws=None, world=1):
    """-> dict(value, cond, gx, gy (d value / dx, dy for THIS rank's elements), Z).  global_ws: the weight sum over all ranks
    (default: this rank's); the masked mean's Z = global_ws / world + 1e-8 with 1e-8 as float32 rounds it."""
    x64 = f64(x)
    s, ws, sabs = loss_stats(kind, x, y, ysign, w)
    Z = float(x64.size) if norm == "mean" else (ws if global_ws is None else global_ws) / world + float(F32(1e-8))
    r = x64 + (0.0 if y is None else ysign * f64(y))
    wv = np.ones(x64.shape[0]) if w is None else f64(w)
    gx = coef / Z * wv[:, None] * _drho(kind, r)
    return dict(value=coef * s / Z, cond=abs(coef) * sabs / Z, gx=gx, gy=ysign * gx, Z=Z, sum=s, ws=ws)


def loss_inputs(rows, cols, seed, regime="plain"):
    """float32 x, y [rows, cols], w [rows].  regimes: "plain" (w in [0, 1) with exact zeros), "zero_w" (w == 0: the masked mean
    divides by Z = 1e-8), "tie" (x == y exactly: residual 0 everywhere)"""
    r = rng(2, rows, cols, seed)
    x = r.standard_normal((rows, cols)).astype(F32)
    y = r.standard_normal((rows, cols)).astype(F32)
    w = r.uniform(0, 1, rows).astype(F32)
    w[r.uniform(0, 1, rows) < 0.25] = 0
    if regime == "zero_w":
        w[:] = 0
    if regime == "tie":
        y = x.copy()
    return x, y, w


# ----------------------------------------------------------------------------------------------------------------------------
# Per-frame median depth loss (k_frame_depth_loss).  Ties rule (the existing GPU test documents it): the median is the LOWER
# middle element; its gradient is shared evenly by the cnt elements equal to it (ATen's evenly_distribute_backward) and
# d|x - med| is 0 at x == med.  Frames with fewer than two selected rays are skipped; frame ids outside [0, T) select nothing.
#   inv = 1 / (mean |x - med| + 1e-10): one rounding per deviation, the block sum (ceil(N / 1024) serial adds, six wave steps, the
#   serial sum of 16 wave partials = c(N) = ceil(N / 1024) + 21), the division by n, + 1e-10, the reciprocal: k_inv = c(N) + 4
#   r = dp inv_p - dg inv_g: dp, dg (1 each, relative to themselves), the products, the difference: (k_inv + 3) on
#   cr = |dp| inv_p + |dg| inv_g.
#   loss = coef sum_k sum_j r^2 / count: 2 (k_inv + 3) through r^2 on |r| cr, then the square and the sums (c(N) + 1, T frames,
#   three for coef * L / c) on r^2:                 k_fdl = 2 (k_inv + 3) + c(N) + T + 4   on  coef / count * sum (|r| cr + r^2)
#   gradient  g_j = coef / count * (2 r_j inv - e_j A inv - B inv^2 / n (sgn_j - e_j Sg)),  A = sum 2 r, B = sum 2 r dp:
#   r and inv^2 carry (k_inv + 3) + 2 k_inv, A and B a block sum each (c(N)), and 12 for the remaining products, differences and
#   the scale g_loss * coef / count * gscale:       k_fdl_grad = 3 k_inv + c(N) + 15      on the same formula with absolute terms
# ----------------------------------------------------------------------------------------------------------------------------
FDL_FRAME_SIZES = (0, 1, 2, 3, 511, 512, 513)      # batches of 1600 rays and more hold all of them ...
FDL_FRAME_SIZES_SMALL = (0, 1, 2, 3, 255, 256, 257)  # ... the batches around the 1024-ray compaction chunk hold these
FDL_BATCHES = (1023, 1024, 1025, 1600)


def fdl_frame_sizes(N):
    return FDL_FRAME_SIZES if N >= 1600 else FDL_FRAME_SIZES_SMALL


def _fdl_c(N):
    return math.ceil(N / 1024) + 21


def k_fdl(N, T):
    return 2 * (_fdl_c(N) + 4 + 3) + _fdl_c(N) + T + 4


def k_fdl_grad(N):
    return 3 * (_fdl_c(N) + 4) + _fdl_c(N) + 15


def fdl_inputs(N, seed, ties=False):
    """pred, gt float32 [N], frame int64 [N], mask bool [N], T.  Frames 0..6 get fdl_frame_sizes(N)[k] rays each (in a seeded
    shuffle, so that every frame's rays lie on both sides of the chunk boundary); four rays get frame id T and four get -1;
    the rest go to frame 7."""
    r = rng(3, N, seed)
    T = 8
    frame = np.full(N, 7, np.int64)
    perm = r.permutation(N)
    o = 0
    for k, sz in enumerate(fdl_frame_sizes(N)):
        frame[perm[o:o + sz]] = k
        o += sz
    frame[perm[o:o + 4]] = T
    frame[perm[o + 4:o + 8]] = -1
    pred = (3.0 * r.standard_normal(N)).astype(F32)
    gt = r.uniform(0, 1, N).astype(F32)
    if ties:   # several values equal to the (lower) median in frames 3, 5 and 6 (3 rays, a power of two, one more), pred and gt alike
        for k in (3, 5, 6):
            i = np.nonzero(frame == k)[0]
            for a in (pred, gt):
                med = np.sort(a[i])[(i.size - 1) >> 1]
                a[i[:3]] = med
    mask = r.uniform(0, 1, N) < 0.7
    return pred, gt, frame, mask, T


def fdl_ref(pred, gt, frame, T, mask=None, coef=1.0):
    """-> dict(value, cond, grad, gcond, count); count == 0 (every frame skipped): value and grad are NaN (0 / 0)"""
    p, q = f64(pred), f64(gt)
    N = p.size
    sel_all = np.ones(N, bool) if mask is None else np.asarray(mask, bool)
    L = Lc = cnt_rays = 0.0
    graw, gc = np.zeros(N), np.zeros(N)
    for k in range(T):
        i = np.nonzero((np.asarray(frame) == k) & sel_all)[0]
        n = i.size
        if n <= 1:
            continue
        def stats(a):
            med = np.sort(a)[(n - 1) >> 1]
            return med, 1.0 / (np.abs(a - med).mean() + 1e-10)
        mp, ip = stats(p[i])
        mg, ig = stats(q[i])
        dp, dg = p[i] - mp, q[i] - mg
        r = dp * ip - dg * ig
        cr = np.abs(dp) * ip + np.abs(dg) * ig
        L += (r * r).sum()
        Lc += (np.abs(r) * cr + r * r).sum()
        cnt_rays += n
        tie = dp == 0
        e = tie / tie.sum()
        sgn = np.sign(dp)
        A, B, Sg = (2 * r).sum(), (2 * r * dp).sum(), sgn.sum()
        Aa, Ba = (2 * cr).sum(), (2 * cr * np.abs(dp)).sum()
        graw[i] = 2 * r * ip - e * A * ip - B * ip * ip / n * (sgn - e * Sg)
        gc[i] = 2 * cr * ip + e * Aa * ip + Ba * ip * ip / n * (np.abs(sgn) + e * np.abs(Sg))
    with np.errstate(divide="ignore", invalid="ignore"):
        return dict(value=np.float64(coef) * L / cnt_rays, cond=abs(coef) * Lc / cnt_rays if cnt_rays else 0.0,
                    grad=np.float64(coef) / cnt_rays * graw, gcond=abs(coef) / cnt_rays * gc if cnt_rays else gc, count=cnt_rays)


# ----------------------------------------------------------------------------------------------------------------------------
# Distortion loss (k_distloss, k_distloss_bwd): per ray  sum_ij w_i w_j |m_i - m_j| + (1/3) sum_i iv_i w_i^2
#   kernel: a wave per ray, tiles of 64 samples, t = ceil(S / 64).  Per sample: w m (1), two six-step wave scans (6), the carry of
#   the earlier tiles (1, itself a sum of t tile totals: t), m P_w (1), the difference (1), the products with w and with 2 (1),
#   the interval term (3), their sum (1), the per-lane sum over tiles (t), the closing wave sum (6):   k_dist = 21 + 2 t
#   backward: the same prefix sums (8 + t), the two totals (t serial + 6 wave steps, then a difference each: t + 8), m (P - Q) and
#   the differences (4), the interval term (2), the sum and the product with g (2):                     k_dist_grad = 24 + 2 t
#   g_w[o] += ...: + half an ulp of the stored sum.
# Condition scales (of the LOSS, not of the prefix form):  sum_ij w_i w_j |m_i - m_j| + iv w^2 / 3  per ray, and
# 2 sum_j w_j |m_i - m_j| + 2/3 iv_i w_i  per sample.  Weights are >= 0, so both equal the values themselves.
# ----------------------------------------------------------------------------------------------------------------------------
DIST_SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 257)
DIST_RAYS = 12


def k_dist(S):
    return 21 + 2 * math.ceil(S / 64)


def k_dist_grad(S):
    return 24 + 2 * math.ceil(S / 64)


def dist_inputs(S, seed):
    """w, m, iv float32 [12, S], m ascending in [0, 1).  ray 0: all weights 0; rays 1, 2: one-hot (first / last tile); rays 3, 4:
    runs of 8 equal midpoints; the rest: w uniform / S with exact zeros"""
    r = rng(4, S, seed)
    N = DIST_RAYS
    w = (r.uniform(0, 1, (N, S)) / S).astype(F32)
    w[r.uniform(0, 1, (N, S)) < 0.2] = 0
    m = np.sort(r.uniform(0, 1, (N, S)), -1).astype(F32)
    w[0] = 0
    w[1] = 0
    w[1, 0] = 1
    w[2] = 0
    w[2, S - 1] = 1
    for n in (3, 4):
        m[n] = m[n, (np.arange(S) // 8) * 8]
    iv = (r.uniform(0.5, 1.5, (N, S)) / S).astype(F32)
    return w, m, iv


def dist_ref(w, m, iv):
    """iv: float or [N, S] -> dict(ray [N], grad [N, S] (of the per-ray loss), cond == ray, gcond == grad)"""
    w, m = f64(w), f64(m)
    iv = np.broadcast_to(f64(F32(iv)) if np.isscalar(iv) else f64(iv), w.shape)
    d = np.abs(m[:, :, None] - m[:, None, :])
    ray = (w[:, :, None] * w[:, None, :] * d).sum((1, 2)) + (iv * w * w).sum(-1) / 3.0
    grad = 2.0 * (w[:, None, :] * d).sum(-1) + (2.0 / 3.0) * iv * w
    return dict(ray=ray, grad=grad, cond=np.abs(ray), gcond=np.abs(grad))


# ----------------------------------------------------------------------------------------------------------------------------
# TV (k_tv_fwd, k_tv_bwd, k_tv_grad) on a (1, C, H, W) view with any strides
#   sums: a difference and its square (2), the serial part of a thread (at most 8: the grid is sized to 2048 elements per
#   block), six wave steps, two levels of the block sum, one float atomic per block (gx blocks):     k_tv_sum = 18 + gx
#   gradient  g = gh (a - b) + gw (a' - b'),  a, b the backward and forward differences: each difference (1), a - b (1), the
#   coefficient, itself rounded (2), the sum of the two directions (1): k_tv_g = 5 on |gh| (|a| + |b|) + |gw| (|a'| + |b'|);
#   through TVLoss the scalar arithmetic around the sums is torch's (2 / count, weight, batch: 4 more).  Stored with +=: half an ulp.
# ----------------------------------------------------------------------------------------------------------------------------
TV_SHAPES = ((4, 1, 1), (4, 2, 1), (4, 1, 2), (3, 5, 7), (16, 33, 9), (48, 9, 33), (12, 64, 1))
TV_LAYOUTS = ("cl_w", "cl_h", "cf")   # channel-last with sW <= sH, channel-last with sW > sH, channel-first (contiguous)
K_TV_G = 5


def k_tv_sum(C, H, W):
    return 18 + max(1, min(512, math.ceil(C * H * W / 2048)))


def tv_tensor(x, layout):
    """a (1, C, H, W) torch view of the values x [C, H, W] in the storage order `layout`"""
    t = torch.as_tensor(x)
    if layout == "cf":
        return t.clone().contiguous()[None]
    if layout == "cl_w":
        return t.permute(1, 2, 0).contiguous().permute(2, 0, 1)[None]
    return t.permute(2, 1, 0).contiguous().permute(2, 1, 0)[None]


def tv_inputs(C, H, W, seed):
    r = rng(5, C, H, W, seed)
    return r.standard_normal((C, H, W)).astype(F32), r.standard_normal((C, H, W)).astype(F32)   # values, gradient pre-fill


def tv_ref(x, ch=1.0, cw=1.0):
    """x [C, H, W] -> dict(sums (h, w), grad = d(ch sum_h + cw sum_w)/dx, gcond)"""
    x = f64(x)
    dh, dw = np.diff(x, axis=1), np.diff(x, axis=2)
    g, gc = np.zeros_like(x), np.zeros_like(x)
    for d, ax, c in ((dh, 1, ch), (dw, 2, cw)):
        pad = [(0, 0)] * 3
        pad[ax] = (1, 0)
        a = np.pad(d, pad)                                        # x[i] - x[i - 1], 0 at i = 0
        pad[ax] = (0, 1)
        b = np.pad(d, pad)                                        # x[i + 1] - x[i], 0 at the end
        g += 2.0 * c * (a - b)
        gc += 2.0 * abs(c) * (np.abs(a) + np.abs(b))
    return dict(sums=np.array([(dh * dh).sum(), (dw * dw).sum()]), grad=g, gcond=gc)


# ----------------------------------------------------------------------------------------------------------------------------
# Dense L1 (k_dense_l1): mean over X x Y x Z of |act(f)|,  f = sum_c P0[c,y,x] L0[c,z] + P1[c,z,x] L1[c,y] + P2[c,z,y] L2[c,x]
#   f: 24 products and their sums (16 + 4 + 4 fused or not, + 2):  26 on cf = sum |terms|.  act: relu exact, softplus
#   (log1pf(expf())) and sigmoid (1 / (1 + expf())) 4 each, both with slope <= 1 / <= 1/4 in f.
#   value: the loop over the third axis (Wn serial adds), six wave steps, two block levels, one float atomic per block (nb):
#       k_l1 = 26 + 4 + Wn + 8 + nb   on  mean(cf + |act|)
#   gradient of a factor entry = gs sum dact(f) * (the other factor): gs = g * 1 / nv (2), s = gs dact (1), the serial fma chain
#   over the loop axis (Wn), for the lines five shuffle steps or eight LDS rows and an atomic per block (8 + nb), stored with +=:
#       k_l1_grad = 26 + 4 + 3 + Wn + 8 + nb   on  gs sum (|dact| + slope * cf) |other factor|,  slope = 1/4 softplus, 0 relu
#   A gradient entry is stored with += once per contributing workgroup: a plane texel by its one owner, a line entry by one float
#   atomic per block along the other thread axis (l1_stores); each store rounds the running sum: l1_stores half ulps of
#   |pre-fill| + |terms|.
#   ReLU's dact is a step: a voxel whose |f| is within 26 * 2^-24 cf of 0 may legitimately fall on either side; its whole term
#   gs |other factor| is added to that entry's bound (l1_ref's `flip`).  The integer regime has f == 0 EXACTLY at many voxels and
#   exact arithmetic in any order: there the step must be 0 (torch: relu'(0) = 0), which the bound above then demands.
# ----------------------------------------------------------------------------------------------------------------------------
L1_GRIDS = ([1, 1, 1], [3, 2, 5], [31, 7, 2], [32, 8, 1], [33, 9, 3], [40, 44, 26])
L1_SHIFT = -1.0


def k_l1(grid, grad=False):
    X, Y, Z = grid
    wn = max(X, Y, Z)
    nb = max(math.ceil(X / 32) * math.ceil(Y / 8), math.ceil(X / 32) * math.ceil(Z / 8), math.ceil(Y / 32) * math.ceil(Z / 8))
    return 26 + 4 + wn + 8 + nb + (3 if grad else 0)


def l1_stores(grid):
    """rounded stores into each of the six gradient tensors: planes 1; L0 (sweep 1) and L1 (sweep 0) one atomic per block in x,
    L2 (sweep 0) one per block in y"""
    X, Y, Z = grid
    return [1, 1, 1, math.ceil(X / 32), math.ceil(X / 32), math.ceil(Y / 8)]


def l1_inputs(grid, seed, regime="normal"):
    """planes P0 [16,Y,X], P1 [4,Z,X], P2 [4,Z,Y]; lines L0 [16,Z], L1 [4,Y], L2 [4,X]; six gradient pre-fills of the same shapes.
    "integer": factors in {-2..2} with a zero row / column of every factor, so that f is a small integer, often exactly 0"""
    X, Y, Z = grid
    r = rng(6, X, Y, Z, seed)
    shapes = [(16, Y, X), (4, Z, X), (4, Z, Y), (16, Z), (4, Y), (4, X)]
    if regime == "integer":
        fs = [r.integers(-2, 3, s).astype(F32) for s in shapes]
        fs[0][:, 0, :] = 0
        fs[1][:, 0, :] = 0
        fs[2][:, 0, :] = 0          # z = 0, y = 0 (P0) ... : whole lines of voxels with few live terms
        fs[3][:, 0] = 0
    else:
        fs = [(0.5 * r.standard_normal(s)).astype(F32) for s in shapes]
    pre = [r.integers(-3, 4, s).astype(F32) if regime == "integer" else r.standard_normal(s).astype(F32) for s in shapes]
    return fs, pre


def l1_ref(fs, act, shift=L1_SHIFT, g=1.0):
    """-> dict(value, cond, f, grads [6] of g * value, gconds [6] (flip allowance included))"""
    P0, P1, P2, L0, L1, L2 = [f64(a) for a in fs]
    A = [np.abs(a) for a in (P0, P1, P2, L0, L1, L2)]

    def vol(p0, p1, p2, l0, l1, l2):
        return np.einsum("cyx,cz->xyz", p0, l0) + np.einsum("czx,cy->xyz", p1, l1) + np.einsum("czy,cx->xyz", p2, l2)
    f, cf = vol(P0, P1, P2, L0, L1, L2), vol(*A)
    nv = f.size
    if act == "relu":
        a, da, slope = np.maximum(f, 0), (f > 0).astype(np.float64), 0.0
        flip = (np.abs(f) <= 26 * U * cf) & (cf > 0) & (f != 0)
    else:
        z = f + shift
        a, da, slope = np.logaddexp(0, z), 1.0 / (1.0 + np.exp(-z)), 0.25
        flip = np.zeros_like(f, bool)
    gs = g / nv

    def back(s, absolute):
        q = A if absolute else (P0, P1, P2, L0, L1, L2)
        return [np.einsum("xyz,cz->cyx", s, q[3]), np.einsum("xyz,cy->czx", s, q[4]), np.einsum("xyz,cx->czy", s, q[5]),
                np.einsum("xyz,cyx->cz", s, q[0]), np.einsum("xyz,czx->cy", s, q[1]), np.einsum("xyz,czy->cx", s, q[2])]
    grads = back(gs * da, False)
    gconds = back(abs(gs) * (np.abs(da) + slope * cf), True)
    flips = back(abs(gs) * flip.astype(np.float64), True)
    return dict(value=np.abs(a).mean(), cond=(cf + np.abs(a)).mean(), f=f, cf=cf, grads=grads, gconds=gconds, flips=flips,
                n_flip=int(flip.sum()))


# ----------------------------------------------------------------------------------------------------------------------------
# Bilinear upsampling, align_corners (k_upsample, ATen's rule): scale = (in - 1) / (out - 1) in float32 (0 for out == 1),
# src = scale * dst in float32, i0 = min(floor(src), in - 1), lambda = src - i0 (exact in float32), i1 = i0 + (i0 < in - 1).
# The index arithmetic is float32 here as in the kernel; only the interpolation is float64:
#   o = (1 - ly)((1 - lx) a + lx b) + ly ((1 - lx) e + lx f): 1 - lx (1), the product (1), the inner sum (1), the outer product
#   with the rounded 1 - ly (2), the outer sum (1):  K_UP = 6  on the same expression with absolute values.
# One more rounding sits in src = scale * dst itself: an evaluation that fuses the product into src - i0 (one fma: the kernel
# behaves so -- inferred from its results and from the pinned point below, not read from its instructions) skips it, ATen does not.  Both are float32 orderings of the rule, and lambda differs between them by
# d = |scale * dst - fl32(scale * dst)|, known per output row / column, plus the rounding of the fused result itself (2^-24 lambda;
# src - i0 of two float32 numbers is exact, the fma's result is rounded once); the bound carries  d_y |do/dly| + d_x |do/dlx|
# (up_ref's `lam`).  It is 0 wherever the product is exact and lambda is 0 (identity resize, extent 1).
# An identity resize has scale 1.0, lambda 0.0 exactly: o = 1 (1 a + 0 b) + 0 (...) = a, bit for bit.
# PINNED points: where fl32(scale * dst) is an integer and the exact product is not above it, ATen's lambda is exactly 0 and the
# fused lambda is 0 or a rounding below 0, which the clamp lifts to 0: on both axes at once the output is the source texel, bit for
# bit (up_ref's `pin`).  157 -> 133 has such a point strictly inside, dst 121: fl32(156 / 132) * 121 rounds to 143.0 from 6.6e-6
# below.  Without the clamp that row moves by 6.6e-6 |b - a|, a hundred half ulps.
# ----------------------------------------------------------------------------------------------------------------------------
K_UP = 6
UP_PAIRS = ((1, 5), (5, 1), (2, 3), (7, 7), (17, 141), (141, 20), (157, 133))


def _up_axis(n_in, n_out):
    scale = F32(n_in - 1) / F32(n_out - 1) if n_out > 1 else F32(0)
    src = (scale * np.arange(n_out, dtype=F32)).astype(F32)
    i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    lam = np.clip((src - i0.astype(F32)).astype(F32), 0, 1).astype(np.float64)
    exact = np.float64(scale) * np.arange(n_out, dtype=np.float64)
    d = np.abs(exact - src.astype(np.float64)) + U * lam
    return i0, i0 + (i0 < n_in - 1), lam, d, (lam == 0) & (exact <= src.astype(np.float64))


def up_pinned_below(n_in, n_out):
    """output indices whose rounded source index is an integer while the exact product scale * dst lies strictly below it"""
    scale = F32(n_in - 1) / F32(n_out - 1) if n_out > 1 else F32(0)
    dst = np.arange(n_out, dtype=np.float64)
    src = (scale * dst.astype(F32)).astype(F32).astype(np.float64)
    return np.nonzero((src == np.floor(src)) & (np.float64(scale) * dst < src))[0]


def up_ref(x, Ho, Wo):
    """x [C, H, W] float32 -> dict(out [C, Ho, Wo], cond, lam: the allowance for the rounding of scale * dst, pin [Ho, Wo]:
    the points whose output is the source texel bit for bit, src: that texel [C, Ho, Wo])"""
    x = f64(x)
    y0, y1, ly, dy, py = _up_axis(x.shape[1], Ho)
    x0, x1, lx, dx, px = _up_axis(x.shape[2], Wo)
    ly, lx = ly[None, :, None], lx[None, None, :]

    def at(v):
        a, b = v[:, y0][:, :, x0], v[:, y0][:, :, x1]
        e, f = v[:, y1][:, :, x0], v[:, y1][:, :, x1]
        return (1 - ly) * ((1 - lx) * a + lx * b) + ly * ((1 - lx) * e + lx * f)
    a, b, e, f = x[:, y0][:, :, x0], x[:, y0][:, :, x1], x[:, y1][:, :, x0], x[:, y1][:, :, x1]
    d_ly = np.abs((1 - lx) * (e - a) + lx * (f - b))
    d_lx = np.abs((1 - ly) * (b - a) + ly * (f - e))
    return dict(out=at(x), cond=at(np.abs(x)), lam=dy[None, :, None] * d_ly + dx[None, None, :] * d_lx,
                pin=py[:, None] & px[None, :], src=a)


# ----------------------------------------------------------------------------------------------------------------------------
# rows_scatter_add (k_rows_scatter_add): g_table[idx[n]] += g_rows[n], indices outside [0, R) skipped.  Small-integer gradients:
# every partial sum is an integer below 2^24, exact in float32 in ANY order, so the comparison is torch.equal.
# ----------------------------------------------------------------------------------------------------------------------------
RSA_CASES = ((1, 1, 1), (12, 12, 4096), (683, 12, 3000), (8192, 1, 5000), (8193, 1, 5000))
RSA_LDS_FLOATS = 8192


def rsa_inputs(R, C, N, seed, out_of_range=True):
    r = rng(7, R, C, N, seed)
    idx = r.integers(0, R, N).astype(np.int64)
    if out_of_range and N >= 8:
        idx[r.permutation(N)[:6]] = [-1, R, -1, R, R + 5, -7]
    g = r.integers(-8, 9, (N, C)).astype(F32)
    pre = r.integers(-8, 9, (R, C)).astype(F32)
    return idx, g, pre


def rsa_ref(idx, g, pre):
    out = f64(pre).copy()
    ok = (idx >= 0) & (idx < out.shape[0])
    np.add.at(out, idx[ok], f64(g)[ok])
    return out
