"""Float64 reference of the whole-scene composition (rdrf_scene_alpha, include/rodynrf.h) and the bounds its fp32 results are
held to; shared by test_scene_volume_cpu.py and test_gpu_scene_volume.py.  No GPU.

The reference takes the fp32 sigma_s, sigma_d, blending and length widened to float64, so both sides see the same values:

    a_d = 1 - exp(-sigma_d length),  a_s = 1 - exp(-sigma_s length)
    w_d = a_d b,  w_s = a_s (1 - b)
    alpha = 1 - (1 - w_d)(1 - w_s)
    owner = w_d / (w_d + w_s), 0 where the sum is 0

The bounds, counted from the kernel's operations (scene_compose and alpha_of, csrc).  u = 2^-24; every quantity below lies in
[0, 1], so one rounding of a result moves it by at most half an ulp of 1, u / 2.

    x = -sigma length     one rounding, relative 2^-24: exp(x) moves by |x| e^x 2^-24 <= u / e          0.37 u
    e = expf(x)           2 ulp of a number <= 1 (the allowance tests/test_gpu_alpha.py makes)         2 u
    a = 1 - e             one rounding                                                                 0.5 u    a: 3 u (2.87)
    nb = 1 - b            one rounding                                                                 0.5 u
    w_d = a_d b           3 u b + one rounding                                                                  w_d: 3.5 u
    w_s = a_s nb          3 u nb + 0.5 u a_s + one rounding                                                     w_s: 4 u
    p = 1 - w_d,  q = 1 - w_s      one rounding each                                                            p: 4 u, q: 4.5 u
    pq                    4 u q + 4.5 u p + one rounding (+ a second-order term of 18 u^2)                      pq: 9 u
    alpha = 1 - pq        one rounding                                                                          alpha: 9.5 u

K_ALPHA = 10 covers it with the second-order term.  The owner: num = w_d carries 3.5 u, den = w_d + w_s carries
3.5 + 4 + 0.5 = 8 u, and the computed quotient is (num + e1) / (den + e2) rounded once, which differs from num / den by
(e1 - owner e2) / (den + e2): at most (3.5 + 8) u / (den - 8 u) + u / 2.  K_OWNER = 12 over the condition scale den - 8 u, plus
u -- the way tests/_hits_prim.py treats the owner of a hit, with the denominator's own error taken off the scale.  Where
den <= 8 u + 12 u the bound exceeds 1 and says nothing: an owner is then only held to [0, 1] (and to exactly 0 where both
weights are exactly 0)."""
import numpy as np

U24 = 2.0 ** -24
K_ALPHA = 10
K_OWNER = 12
DEN_ERR = 8     # units of u on w_d + w_s
ORDER = ("alpha", "owner", "sigma_s", "sigma_d", "blending")   # alpha.SCENE_OUTPUTS

DEFECTS = ("swap_b", "keep_eps", "a_s_from_sigma_d")


def compose(sigma_s, sigma_d, b, length, dtype=np.float64, defect=None):
    """the composition in `dtype`, in the kernel's order (float64: the reference; float32: the kernel's arithmetic restated
    with numpy's one-rounding operations) -> (alpha, owner, den).  defect: one of DEFECTS, planted"""
    f = dtype
    ss, sd, b, ln = (np.asarray(v).astype(f) for v in (sigma_s, sigma_d, b, length))
    one = f(1.0)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        a_d = one - np.exp((-sd * ln).astype(f)).astype(f)
        a_s = one - np.exp((-(sd if defect == "a_s_from_sigma_d" else ss) * ln).astype(f)).astype(f)
        if defect == "swap_b":
            b = (one - b).astype(f)
        w_d = (a_d * b).astype(f)
        nb = (one - b).astype(f)
        w_s = (a_s * nb).astype(f)
        pq = ((one - w_d).astype(f) * (one - w_s).astype(f)).astype(f)
        if defect == "keep_eps":
            pq = (pq + f(1e-10)).astype(f)
        alpha = (one - pq).astype(f)
        den = (w_d + w_s).astype(f)
        owner = np.where(den == 0, f(0.0), w_d / np.where(den == 0, one, den)).astype(f)
    return alpha, owner, den


def alpha_bound():
    return K_ALPHA * U24


def owner_bound(den):
    """per entry; inf where the denominator is within its own error of 0"""
    den = np.asarray(den, dtype=np.float64)
    scale = den - DEN_ERR * U24
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(scale > 0, K_OWNER * U24 / np.where(scale > 0, scale, 1.0) + U24, np.inf)


def check(alpha, owner, sigma_s, sigma_d, b, length):
    """fp32 alpha / owner against the float64 reference on the same ingredients -> (worst alpha error / bound, worst owner
    error / bound over the entries whose bound is finite, ok).  NaN ingredients: NaN expected in both, exactly there."""
    ra, ro, den = compose(sigma_s, sigma_d, b, length)
    alpha, owner = np.asarray(alpha, dtype=np.float64), np.asarray(owner, dtype=np.float64)
    nan = np.isnan(ra)
    ok = np.array_equal(np.isnan(alpha), nan) and np.array_equal(np.isnan(owner), nan)
    fin = ~nan
    ea = np.abs(alpha - ra)[fin] / alpha_bound()
    ob = owner_bound(den)
    sel = fin & np.isfinite(ob)
    eo = (np.abs(owner - ro)[sel] / ob[sel]) if sel.any() else np.zeros(0)
    loose = fin & ~np.isfinite(ob)
    ok = ok and bool(((owner[loose] >= 0) & (owner[loose] <= 1)).all()) and bool((owner[fin & (den == 0)] == 0).all())
    return (float(ea.max()) if ea.size else 0.0), (float(eo.max()) if eo.size else 0.0), ok


def ingredients(n, seed, length=0.08):
    """seeded fp32 (sigma_s, sigma_d, b): optical depths sigma length log-uniform over 1e-5 .. 50 (thin media to walls), a fifth of
    the entries with one sigma exactly 0, a twentieth with both, blending exactly 0, exactly 1 or 2^-126 in 10 % of the entries
    each"""
    g = np.random.default_rng(seed)
    depth = lambda: 10.0 ** g.uniform(-5.0, 1.7, n) / length
    ss, sd = depth(), depth()
    kind = g.random(n)
    ss = np.where((kind < 0.2) | (kind > 0.95), 0.0, ss)
    sd = np.where((kind > 0.75), 0.0, sd)
    b = g.random(n)
    kb = g.random(n)
    b = np.where(kb < 0.1, 0.0, np.where(kb < 0.2, 1.0, np.where(kb < 0.3, 2.0 ** -126, b)))
    return ss.astype(np.float32), sd.astype(np.float32), b.astype(np.float32)
