"""Float64 references, seeded generators and error bounds for the ray geometry kernels of csrc/rdrf_misc.hip and
csrc/rdrf_misc_dev.hpp: k_generate_rays / _bwd, k_sample_ndc / _contract / _world, k_sample_bwd, k_sample_world_bwd, k_induce_flow /
_bwd.  Shared by test_geom_primitives_cpu.py (keeps these references honest against the oracle in float64, torch autograd and the
fixtures, and shows that a float32 oracle evaluation meets every bound) and test_gpu_geom_primitives.py (holds the kernels to them).

Every reference takes the SAME float32 inputs the kernel gets, widens them to float64 and restates the kernel's operations one by
one on `V` objects: a float64 value v, a bound e on |computed - v| and r, the largest relative bound e(b) / |b| of any divisor (or
square-root argument) in the history of the element.  The constants the kernels round to float32 (cx, cy, kw, kh, c, c2, inv_far,
1e-6f, 1 - 1e-6f, 256, -2 / W) enter as those float32 values.  The adjoints are written out by hand on the same objects (no autograd
here; the CPU file compares them with autograd).  Rules, u = 2^-24 per rounded operation:

    e(a + b) = u |a + b| + e(a) + e(b)                      e(a b) = u |a b| + |a| e(b) + |b| e(a) + e(a) e(b)
    e(a / b) = u |a / b| + e(a) / |b| + |a| e(b) / b^2      e(sqrt a) = u sqrt(a) + e(a) / (2 sqrt a)
    e(sum of n terms through `depth` additions) = sum e(t_i) + depth u sum |t_i|

Exact operations (negation, products with powers of two, selections, the clamp where it holds) add nothing.  A fused multiply-add
rounds once where the rule above counts twice: the bound covers contracted and uncontracted builds alike.  The sums over the
samples of a ray are lane-strided and closed by six wave steps: depth ceil(S / 64) + 6.  The atomic sums over rays (g_poses per
view, g_focal) come in ARBITRARY order: depth = the number of contributing (non-zero) rays, which with the pre-filled value is the
deepest tree their additions can form (additions of an exact zero are exact).  Stored results get half an ulp on top.

SECOND-ORDER TERMS.  Kept: e(a) e(b) of a product.  Dropped: the factor 1 / (1 - rho) of every division and square root (the exact
bound of a / b is (e(a) + |a / b| e(b)) / (|b| - e(b)), rho = e(b) / |b|), and the u e of rounding a perturbed result.  At most ten
divisions by a perturbed divisor lie on any path of these kernels (ray generation: n1, n2, d_z, o_z forward and o_z^2, d_z, n2,
n1 in the adjoint; flow: the contraction norm twice, c - 1 or m (2 - m), cam_z forward and each once more, squared, backward), and
the generators allow no divisor a relative first-order bound above RHO_LIMIT = 2^-4 (elements above it are checked for finiteness
only: the near-singular sets; the ordinary sets stay below RHO_ORDINARY = 2^-10):  (1 - 2^-4)^-10 = 1.907 < SECOND = 2.
Every bound the tests use is SECOND * e (+ half an ulp where stored).

DISCRETE CHOICES (the arg-max component of an L-inf norm, nrm > 1, the clamp of P.z, raw against near / far, the slab and axis of
t_min, `valid` at a face): each reference returns the float64 margin of every decision it took next to the propagated bound of
the compared quantity; the generators redraw (seeded) until every margin exceeds SECOND * bound, so the reference and the kernel
cannot disagree.  The cases built ON a tie or a face are exact in float32 by construction and compared bit for bit."""
import math
import zlib

import numpy as np

from _step_prim import F32, U, f64, half_ulp, rng  # noqa: F401

SECOND = 2.0
RHO_LIMIT = 2.0 ** -4
RHO_ORDINARY = 2.0 ** -10
_EXACT = [False]


class exact_consts:
    """inside: the constants the kernels round to float32 keep their float64 values (the form the float64 oracle computes)"""
    def __enter__(self):
        _EXACT[0] = True

    def __exit__(self, *a):
        _EXACT[0] = False


def c32(x32, x64=None):
    """a kernel constant: its float32 value, or (inside exact_consts) the float64 value it stands for"""
    return float(x32 if x64 is None else x64) if _EXACT[0] else float(F32(x32))


def eps6():
    return c32(1e-6)


def clamp_hi():
    return c32(F32(1.0) - F32(1e-6), 1.0 - 1e-6)


# ----------------------------------------------------------------------------------------------------------------------------
# value / bound / divisor-bound arithmetic
# ----------------------------------------------------------------------------------------------------------------------------
class V:
    __slots__ = ("v", "e", "r")

    def __init__(self, v, e=0.0, r=0.0):
        self.v = np.asarray(v, np.float64)
        self.e = np.zeros(self.v.shape) + np.asarray(e, np.float64)
        self.r = np.zeros(self.v.shape) + np.asarray(r, np.float64)

    @staticmethod
    def of(x):
        return x if isinstance(x, V) else V(x)

    def _rnd(self, v, e, r):
        with np.errstate(invalid="ignore"):
            return V(v, e + U * np.abs(v), r)

    def __add__(self, o):
        o = V.of(o)
        return self._rnd(self.v + o.v, self.e + o.e, np.maximum(self.r, o.r))

    __radd__ = __add__

    def __sub__(self, o):
        o = V.of(o)
        return self._rnd(self.v - o.v, self.e + o.e, np.maximum(self.r, o.r))

    def __rsub__(self, o):
        return V.of(o) - self

    def __mul__(self, o):
        o = V.of(o)
        with np.errstate(invalid="ignore"):
            return self._rnd(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e, np.maximum(self.r, o.r))

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = V.of(o)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = self.v / o.v
            return self._rnd(q, self.e / np.abs(o.v) + np.abs(self.v) * o.e / (o.v * o.v),
                             np.maximum(np.maximum(self.r, o.r), o.e / np.abs(o.v)))

    def __rtruediv__(self, o):
        return V.of(o) / self

    def __neg__(self):
        return V(-self.v, self.e, self.r)

    def x2(self, c):
        """exact product with a power of two (or a sign)"""
        return V(self.v * c, self.e * abs(c), self.r)

    def sqrt(self):
        with np.errstate(divide="ignore", invalid="ignore"):
            s = np.sqrt(self.v)
            return self._rnd(s, self.e / (2.0 * s), np.maximum(self.r, self.e / np.abs(self.v)))

    def abs(self):
        return V(np.abs(self.v), self.e, self.r)

    def __getitem__(self, i):
        return V(self.v[i], self.e[i], self.r[i])

    def reshape(self, *s):
        return V(self.v.reshape(*s), self.e.reshape(*s), self.r.reshape(*s))

    @property
    def bound(self):
        return SECOND * self.e


def where(c, a, b):
    a, b = V.of(a), V.of(b)
    return V(np.where(c, a.v, b.v), np.where(c, a.e, b.e), np.where(c, a.r, b.r))


def fma(a, b, c):
    """one rounding: a b + c"""
    a, b, c = V.of(a), V.of(b), V.of(c)
    v = a.v * b.v + c.v
    return V(v, np.abs(a.v) * b.e + np.abs(b.v) * a.e + a.e * b.e + c.e + U * np.abs(v), np.maximum(np.maximum(a.r, b.r), c.r))


def vsum(x, axis, depth):
    """a sum whose terms pass through at most `depth` additions"""
    return V(x.v.sum(axis), x.e.sum(axis) + depth * U * np.abs(x.v).sum(axis), x.r.max(axis) if x.v.shape[axis] else 0.0)


def lane_depth(S):
    return math.ceil(S / 64) + 6


def dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def pick(lst, k):
    return V(np.choose(k, [x.v for x in lst]), np.choose(k, [x.e for x in lst]), np.choose(k, [x.r for x in lst]))


def argmax3(p):
    """(k, |p_k|, margin, bound): the arg-max component as the kernels pick it (first of equals), the float64 gap to the runner-up
    and the sum of the two bounds it must exceed"""
    a = np.stack([np.abs(x.v) for x in p])
    e = np.stack([x.e for x in p])
    k = np.argmax(a, 0)
    top = np.take_along_axis(a, k[None], 0)[0]
    a2 = a.copy()
    np.put_along_axis(a2, k[None], -1.0, 0)
    k2 = np.argmax(a2, 0)
    gap = top - np.take_along_axis(a2, k2[None], 0)[0]
    eb = np.take_along_axis(e, k[None], 0)[0] + np.take_along_axis(e, k2[None], 0)[0]
    return k, pick(p, k).abs(), gap, eb


def scatter_sum(contrib, index, size, pre):
    """atomic sum in arbitrary order: out[index[n]] = pre + sum_n contrib[n]; depth = the number of non-zero contributions"""
    val = f64(pre).copy()
    np.add.at(val, index, contrib.v)
    mag, err, cnt, rr = np.abs(f64(pre)), np.zeros(size), np.zeros(size), np.zeros(size)
    np.add.at(mag, index, np.abs(contrib.v))
    np.add.at(err, index, contrib.e)
    np.add.at(cnt, index, (contrib.v != 0).astype(np.float64))
    np.maximum.at(rr, index, contrib.r)
    return V(val, err + cnt * U * mag + half_ulp(val) / SECOND, rr)


def accumulate(pre, x):
    """a stored `+=` onto a pre-filled float32 value"""
    s = V(f64(pre)) + x
    return V(s.v, s.e + half_ulp(s.v) / SECOND, s.r)


def bound_ratio(got, ref, skip=None):
    """max |got - ref.v| / (SECOND ref.e) over the elements; a zero bound demands exactness; `skip`: finiteness only"""
    got = f64(got).reshape(ref.v.shape)
    if not np.isfinite(got).all():
        return math.inf
    err, tol = np.abs(got - ref.v), ref.bound
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err > 0, np.inf, 0.0))
    if skip is not None:
        r = np.where(skip, 0.0, r)
    return float(np.nanmax(r)) if r.size else 0.0


def margins_ok(margins):
    """[(name, margin, bound)]: every float64 decision margin above SECOND * bound"""
    return all(bool((np.asarray(m) > SECOND * np.asarray(b)).all()) for _, m, b in margins)


def skey(name):
    """a string as an entry of a seed key"""
    return zlib.crc32(name.encode())


def until_ok(make, *key, tries=200):
    """the first seeded draw whose decision margins all hold"""
    for a in range(tries):
        case = make(rng(*key, a))
        if case is not None and margins_ok(case["margins"]):
            return case
    raise AssertionError(f"no draw with safe decision margins for {key}")


# ----------------------------------------------------------------------------------------------------------------------------
# Ray generation (k_generate_rays, k_generate_rays_bwd)
# ----------------------------------------------------------------------------------------------------------------------------
GRB_LDS_POSES = 448
RAYGEN_N = (1, 255, 256, 257, 1000)
RAYGEN_T = (1, 5, 448, 449)
RAYGEN_SHIFTS = (0, 1, -1, 3, -3)


def raygen_views(ids, view_shift, T, H, W):
    ids = np.asarray(ids, np.int64)
    return np.clip(ids // (W * H) + view_shift, 0, T - 1), ids % W, (ids // W) % H


def raygen_ref(ids, uv, view_shift, poses, focal, H, W, ndc, near, g_rays=None, pre_poses=None, pre_focal=None):
    """-> dict(rays V [N,6]; with g_rays: g_poses V [T,9], g_focal V [1], per_ray contributions)"""
    T = poses.shape[0]
    view, col, row = raygen_views(ids, view_shift, T, H, W)
    f = V(float(F32(focal)))
    pi = V(uv[:, 0]) if uv is not None else V(col + 0.5)
    pj = V(uv[:, 1]) if uv is not None else V(row + 0.5)
    cx, cy = float(F32(W / 2)), float(F32(H / 2))
    dr = [(pi - cx) / f, -((pj - cy) / f)]
    p = [V(f64(poses)[view, k]) for k in range(9)]
    n1 = ((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]).sqrt()
    b1 = [p[k] / n1 for k in range(3)]
    dt = dot3(b1, p[3:6])
    u = [p[3 + k] - dt * b1[k] for k in range(3)]
    n2 = ((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]).sqrt()
    b2 = [u[k] / n2 for k in range(3)]
    b3 = [b1[1] * b2[2] - b1[2] * b2[1], b1[2] * b2[0] - b1[0] * b2[2], b1[0] * b2[1] - b1[1] * b2[0]]
    d = [(dr[0] * b1[k] + dr[1] * b2[k]) + (-b3[k]) for k in range(3)]
    o = p[6:9]
    nr = float(F32(near))
    out_o, out_d = o, d
    if ndc:
        f32 = F32(focal)
        kw = c32(F32(-1.0) / (F32(W) / (F32(2.0) * f32)), -2.0 * float(f32) / W)
        kh = c32(F32(-1.0) / (F32(H) / (F32(2.0) * f32)), -2.0 * float(f32) / H)
        t = -((nr + o[2]) / d[2])
        op = [o[k] + t * d[k] for k in range(3)]
        out_o = [kw * op[0] / op[2], kh * op[1] / op[2], 1.0 + V(2.0 * nr) / op[2]]
        out_d = [kw * (d[0] / d[2] - op[0] / op[2]), kh * (d[1] / d[2] - op[1] / op[2]), V(-2.0 * nr) / op[2]]
    rays = out_o + out_d
    res = dict(rays=V(np.stack([x.v for x in rays], -1), np.stack([x.e for x in rays], -1), np.stack([x.r for x in rays], -1)),
               view=view, dz=d[2], n2=n2)
    if g_rays is None:
        return res
    g = f64(g_rays)
    go, gd = [V(g[:, k]) for k in range(3)], [V(g[:, 3 + k]) for k in range(3)]
    gf = V(np.zeros(len(view)))
    if ndc:
        # the adjoint's own float32 constants: kw = -2 f / W stands for the forward's -1 / (W / (2 f)); the reference keeps the
        # forward's value and carries the difference as a bound
        kwb, khb = c32(F32(-2.0) * f32 / F32(W), kw), c32(F32(-2.0) * f32 / F32(H), kh)
        kwv, khv = V(kw, abs(kwb - kw)), V(kh, abs(khb - kh))
        c_w, c_h = c32(F32(-2.0) / F32(W), -2.0 / W), c32(F32(-2.0) / F32(H), -2.0 / H)
        aa, bb, ra, rb = op[0] / op[2], op[1] / op[2], d[0] / d[2], d[1] / d[2]
        g_kw = go[0] * aa + gd[0] * (ra - aa)
        g_kh = go[1] * bb + gd[1] * (rb - bb)
        gf = gf + (g_kw * c_w + g_kh * c_h)
        g_a, g_b = kwv * (go[0] - gd[0]), khv * (go[1] - gd[1])
        g_ra, g_rb = kwv * gd[0], khv * gd[1]
        op22 = op[2] * op[2]
        gop = [g_a / op[2], g_b / op[2],
               (-((g_a * aa + g_b * bb) / op[2]) - V(2.0 * nr) * go[2] / op22) + V(2.0 * nr) * gd[2] / op22]
        gdd = [g_ra / d[2], g_rb / d[2], -((g_ra * ra + g_rb * rb) / d[2])]
        g_t = dot3(gop, d)
        gdd = [gdd[k] + t * gop[k] for k in range(3)]
        go = [gop[0], gop[1], gop[2] + (-(g_t / d[2]))]
        gdd[2] = gdd[2] + (-(g_t * t / d[2]))
        gd = gdd
    gb1 = [dr[0] * gd[k] for k in range(3)]
    gb2 = [dr[1] * gd[k] for k in range(3)]
    gb3 = [-gd[k] for k in range(3)]
    gdir = [dot3(gd, b1), dot3(gd, b2)]
    gf = gf + (-(gdir[0] * dr[0] / f) - gdir[1] * dr[1] / f)
    cr1 = [b2[1] * gb3[2] - b2[2] * gb3[1], b2[2] * gb3[0] - b2[0] * gb3[2], b2[0] * gb3[1] - b2[1] * gb3[0]]
    cr2 = [gb3[1] * b1[2] - gb3[2] * b1[1], gb3[2] * b1[0] - gb3[0] * b1[2], gb3[0] * b1[1] - gb3[1] * b1[0]]
    gb1 = [gb1[k] + cr1[k] for k in range(3)]
    gb2 = [gb2[k] + cr2[k] for k in range(3)]
    dot2 = dot3(gb2, b2)
    gu = [(gb2[k] - dot2 * b2[k]) / n2 for k in range(3)]
    g_dt = -((gu[0] * b1[0] + gu[1] * b1[1]) + gu[2] * b1[2])
    gb1 = [(gb1[k] - dt * gu[k]) + g_dt * p[3 + k] for k in range(3)]
    gp1 = [gu[k] + g_dt * b1[k] for k in range(3)]
    dot1 = dot3(gb1, b1)
    contrib = [(gb1[k] - dot1 * b1[k]) / n1 for k in range(3)] + gp1 + go
    pre_p = np.zeros((T, 9)) if pre_poses is None else f64(pre_poses)
    cols = [scatter_sum(contrib[k], view, T, pre_p[:, k]) for k in range(9)]
    res["g_poses"] = V(np.stack([c.v for c in cols], -1), np.stack([c.e for c in cols], -1), np.stack([c.r for c in cols], -1))
    res["g_focal"] = scatter_sum(gf, np.zeros(len(view), np.int64), 1, np.zeros(1) if pre_focal is None else f64(pre_focal))
    res["contrib"], res["gf"] = contrib, gf
    return res


def _norms(r, T):
    """|p[0:3]| from 0.1 to 10: both ends present once T >= 2"""
    return (10.0 ** r.permutation(np.linspace(-1, 1, T)))[:, None] if T > 1 else 10.0 ** r.uniform(-1, 1, (1, 1))


def _pose_rows(r, T, regime="plain"):
    """[T,9] float32: 6-D rows NOT normalised (|p[0:3]| from 0.1 to 10); "skew": p[3:6] within a few degrees of p[0:3]"""
    a = r.standard_normal((T, 3))
    a *= _norms(r, T) / np.linalg.norm(a, axis=-1, keepdims=True)
    b = r.standard_normal((T, 3))
    if regime == "skew":
        b = a * r.uniform(1.0, 2.0, (T, 1)) + 0.05 * np.linalg.norm(a, axis=-1, keepdims=True) * b / np.linalg.norm(b, axis=-1, keepdims=True)
    else:
        b *= 10.0 ** r.uniform(-1, 1, (T, 1))
    return np.concatenate([a, b, r.uniform(-0.3, 0.3, (T, 3))], -1).astype(F32)


def _camera_rows(r, T, tilt=0.25):
    """6-D rows of cameras that look down -z up to a tilt (NDC rays need d_z away from 0), un-normalised"""
    a = np.array([1.0, 0, 0]) + tilt * r.standard_normal((T, 3))
    b = np.array([0, 1.0, 0]) + tilt * r.standard_normal((T, 3))
    a *= _norms(r, T) / np.linalg.norm(a, axis=-1, keepdims=True)
    b *= 10.0 ** r.uniform(-1, 1, (T, 1))
    return np.concatenate([a, b, r.uniform(-0.3, 0.3, (T, 3))], -1).astype(F32)


def raygen_case(N, T, ndc, use_uv, view_shift=0, ids_mode="spread", poses="plain", H=24, W=40, seed=0, dead_view=True):
    """ids_mode: "spread" (all views), "one" (one view: the largest same-address contention), "ends" (first and last frame:
    view_shift meets its clamp), "big" (T = 200, H = W = 4096: ids above 2^31).  dead_view: the rays of one view get
    g_rays == 0.  Pre-fills are non-zero."""
    def make(r):
        focal = F32(0.5 * max(H, W) * 1.7320508)
        near = 1.0
        if ids_mode == "big":
            view = np.r_[r.integers(128, T, N - N // 4), r.integers(0, T, N // 4)]
        elif ids_mode == "one":
            view = np.full(N, T // 2)
        elif ids_mode == "ends":
            view = np.where(np.arange(N) % 2 == 0, 0, T - 1)
        else:
            view = np.arange(N) % T if N >= T else r.integers(0, T, N)
        ids = (view.astype(np.int64) * H + r.integers(0, H, N)) * W + r.integers(0, W, N)
        uv = None
        if use_uv:   # several image widths outside the frame as well
            uv = np.stack([r.uniform(-3 * W, 4 * W, N), r.uniform(-3 * H, 4 * H, N)], -1).astype(F32)
        # (NDC rays need d_z away from 0: the cameras of the far-outside uv tilt less)
        P = _camera_rows(r, T, 0.04 if use_uv else 0.25) if ndc and poses == "plain" else _pose_rows(r, T, poses)
        if ndc and poses == "skew":
            P = _camera_rows(r, T, 0.1)
            P[:, 3:6] = (P[:, 0:3] * r.uniform(1.0, 2.0, (T, 1)) + 0.05 * np.linalg.norm(P[:, 0:3], axis=-1, keepdims=True)
                         * np.array([0, 1.0, 0]) * r.uniform(0.5, 1.5, (T, 1))).astype(F32)
        g = r.standard_normal((N, 6)).astype(F32)
        eff = raygen_views(ids, view_shift, T, H, W)[0]
        dead = int(eff[-1]) if dead_view and len(np.unique(eff)) > 1 else -1
        g[eff == dead] = 0
        pre_p, pre_f = r.standard_normal((T, 9)).astype(F32), r.standard_normal(1).astype(F32)
        c = dict(ids=ids, uv=uv, view_shift=view_shift, poses=P, focal=focal, H=H, W=W, T=T, ndc=ndc, near=near, g=g, pre_p=pre_p,
                 pre_f=pre_f, dead=dead, eff=eff, margins=[])
        ref = raygen_ref(ids, uv, view_shift, P, focal, H, W, ndc, near, g, pre_p, pre_f)
        rho = max(ref["rays"].r.max(), ref["g_poses"].r.max(), ref["g_focal"].r.max())
        c["margins"] = [("divisor bounds", RHO_ORDINARY * np.ones(1), rho / SECOND * np.ones(1))]
        c["ref"] = ref
        return c
    return until_ok(make, 20, N, T, int(ndc), int(use_uv), view_shift + 8, skey(ids_mode), skey(poses), H, seed)


def raygen_cases():
    """(tag, kwargs): the ordinary sets"""
    out = []
    for ndc in (False, True):
        for use_uv in (False, True):
            for N in RAYGEN_N:
                out.append((f"N={N}", dict(N=N, T=5, ndc=ndc, use_uv=use_uv)))
            for T in RAYGEN_T:
                out.append((f"T={T}", dict(N=257, T=T, ndc=ndc, use_uv=use_uv)))
            out.append(("one view", dict(N=1000, T=5, ndc=ndc, use_uv=use_uv, ids_mode="one")))
            out.append(("one view T=449", dict(N=257, T=449, ndc=ndc, use_uv=use_uv, ids_mode="one")))
            for s in RAYGEN_SHIFTS[1:]:
                out.append((f"shift={s}", dict(N=257, T=5, ndc=ndc, use_uv=use_uv, view_shift=s, ids_mode="ends")))
            out.append(("ids > 2^31", dict(N=257, T=200, ndc=ndc, use_uv=use_uv, ids_mode="big", H=4096, W=4096)))
            out.append(("skew rows", dict(N=257, T=5, ndc=ndc, use_uv=use_uv, poses="skew")))
    return [(f"raygen {'ndc' if k['ndc'] else 'world'} {'uv' if k['use_uv'] else 'ids'} {t}", k) for t, k in out]


def raygen_singular_case(N=448, T=448, H=24, W=40):
    """ndc rays whose |d_z| runs log-uniformly from 1 down to 2^-15: uv is solved (in float64, then rounded) so that the
    direction's z component hits the target (2^-15 .. 1).  Elements whose divisor bound exceeds RHO_LIMIT are checked for finiteness only.
    ONE RAY PER VIEW (T = N = GRB_LDS_POSES, two workgroups): a row of g_poses then carries the divisor bound of its own ray alone,
    so that the adjoint is held to the bound on every row but those of the over-limit rays.  g_focal is the sum over ALL rays, the
    over-limit ones included: its bound is not meaningful on this set and it is checked for finiteness only."""
    assert T == N
    r = rng(21, N, T)
    focal = F32(0.5 * max(H, W) * 1.7320508)
    P = _camera_rows(r, T, 0.5)
    view = r.permutation(N)
    ids = (view.astype(np.int64) * H + r.integers(0, H, N)) * W + r.integers(0, W, N)
    p = f64(P)[view]
    b1 = p[:, :3] / np.linalg.norm(p[:, :3], axis=-1, keepdims=True)
    u = p[:, 3:6] - (b1 * p[:, 3:6]).sum(-1, keepdims=True) * b1
    b2 = u / np.linalg.norm(u, axis=-1, keepdims=True)
    b3 = np.cross(b1, b2)
    target = -(2.0 ** r.uniform(-15, 0, N))
    vy = r.uniform(0, H, N)
    d1 = -(vy - H / 2) / float(focal)
    d0 = (target + b3[:, 2] - d1 * b2[:, 2]) / b1[:, 2]
    uv = np.stack([d0 * float(focal) + W / 2, vy], -1).astype(F32)
    g = r.standard_normal((N, 6)).astype(F32)
    pre_p, pre_f = r.standard_normal((T, 9)).astype(F32), r.standard_normal(1).astype(F32)
    c = dict(ids=ids, uv=uv, view_shift=0, poses=P, focal=focal, H=H, W=W, T=T, ndc=True, near=1.0, g=g, pre_p=pre_p, pre_f=pre_f,
             dead=-1, margins=[])
    c["ref"] = raygen_ref(ids, uv, 0, P, focal, H, W, True, 1.0, g, pre_p, pre_f)
    return c


# ----------------------------------------------------------------------------------------------------------------------------
# Samplers, forward (sample_ndc_body, sample_contract_body, sample_world_body)
# ----------------------------------------------------------------------------------------------------------------------------
SAMPLE_S = (1, 2, 3, 64, 65, 270)
SAMPLE_BWD_S = (1, 63, 64, 65, 270)
BOX = np.array([[-1.5, -1.67, -1.0], [1.5, 1.67, 1.0]], F32)
WBOX = np.array([[-1.0, -1.25, -0.75], [1.0, 1.25, 0.75]], F32)


def linspace_ref(start, end, steps, idx):
    """ATen's CPU linspace as linspace_at restates it: one fused multiply-add per element"""
    idx = np.asarray(idx, np.float64)
    if steps <= 1:
        return V(np.full(idx.shape, float(start)))
    step = (V(float(end)) - float(start)) / float(steps - 1)
    lo = fma(step, idx, float(start))
    hi = fma(-step, steps - idx - 1, float(end))
    return where(idx < steps // 2, lo, hi)


def _points(rays, t, contract=False):
    """o + d t per component -> list of three V [N,S]; t V [S] or [N,S]"""
    o, d = [V(f64(rays)[:, k, None]) for k in range(3)], [V(f64(rays)[:, 3 + k, None]) for k in range(3)]
    return [o[k] + d[k] * t for k in range(3)]


def _stack(p):
    return V(np.stack([x.v for x in p], -1), np.stack([x.e for x in p], -1), np.stack([x.r for x in p], -1))


def _box_mask(p, box):
    """float64 mask and, per sample, the smallest (distance to a face - bound of that coordinate)"""
    lo, hi = f64(box)[0], f64(box)[1]
    inside = np.ones(p[0].v.shape, bool)
    clear = np.full(p[0].v.shape, np.inf)
    for k in range(3):
        inside &= ~((lo[k] > p[k].v) | (p[k].v > hi[k]))
        clear = np.minimum(clear, np.minimum(np.abs(p[k].v - lo[k]), np.abs(p[k].v - hi[k])) - SECOND * p[k].e)
    return inside, clear


def sample_ndc_ref(rays, S, near, far, jitter, box):
    near, far = F32(near), F32(far)
    t = linspace_ref(near, far, S, np.arange(S))
    if jitter is not None:
        c = c32((float(far) - float(near)) / S)
        t = t + V(f64(jitter)) * c
    p = _points(rays, t)
    inside, clear = _box_mask(p, box)
    N = rays.shape[0]
    return dict(xyz=_stack(p), z=V(np.tile(t.v, (N, 1)), np.tile(t.e, (N, 1))), valid=inside, clear=clear, margins=[])


def contract_t_ref(S, near, far, jin, jout):
    near, far = F32(near), F32(far)
    inner, outer = S - S // 2, S // 2
    j = np.arange(inner)
    a = linspace_ref(near, 2.0, inner + 1, j)
    b = linspace_ref(near, 2.0, inner + 1, j + 1)
    if jin is not None:
        c = c32((2.0 - float(near)) / inner)
        ji = f64(jin)
        a = a + V(ji[j]) * c
        b = where(j + 1 < inner, b + V(ji[np.minimum(j + 1, len(ji) - 1)]) * c, b)
    ti = (b + a).x2(0.5)
    k = np.arange(outer)
    r0, r1 = V((outer - k).astype(np.float64)), V((outer - k - 1).astype(np.float64))
    if jout is not None:
        jo = f64(jout)
        r0 = where(outer - k < outer, r0 + V(jo[np.minimum(outer - k, len(jo) - 1)]), r0)
        r1 = r1 + V(jo[outer - k - 1])
    mid = (r1 + r0).x2(0.5)
    c2, inv_far = c32(0.5 - 1.0 / float(far)), c32(1.0 / float(far))
    to = 1.0 / (inv_far + (c2 * mid) / float(max(outer, 1)))
    return V(np.r_[ti.v, to.v], np.r_[ti.e, to.e], np.r_[ti.r, to.r])


def contract_points(p):
    """the L-inf contraction of ray_point -> (points, nrm, margins)"""
    k, nrm, gap, eb = argmax3(p)
    big = nrm.v > 1.0
    safe = where(big, nrm, 1.0)
    sc = 2.0 - 1.0 / safe
    q = [where(big, sc * (p[i] / safe), p[i]) for i in range(3)]
    return q, k, nrm, big, [("nrm > 1", np.abs(nrm.v - 1.0), nrm.e)], ("arg-max", gap, eb)


def sample_contract_ref(rays, S, near, far, jin, jout):
    t = contract_t_ref(S, near, far, jin, jout)
    q, _, nrm, big, margins, _ = contract_points(_points(rays, t))
    N = rays.shape[0]
    return dict(xyz=_stack(q), z=V(np.tile(t.v, (N, 1)), np.tile(t.e, (N, 1))), valid=np.ones(nrm.v.shape, bool), big=big,
                clear=np.full(nrm.v.shape, np.inf), margins=margins)


def world_tmin_ref(rays, box, near, far):
    """-> dict(t_min, raw V [N], axis, upper, margins): the selected slab quotient and how far every decision is from flipping"""
    R = f64(rays)
    lo, hi = f64(box)[0], f64(box)[1]
    ms, ups, gaps = [], [], []
    for k in range(3):
        vec = V(np.where(R[:, 3 + k] == 0.0, eps6(), R[:, 3 + k]))
        ra, rb = (hi[k] - V(R[:, k])) / vec, (lo[k] - V(R[:, k])) / vec
        up = ra.v < rb.v
        ms.append(where(up, ra, rb))
        ups.append(up)
        gaps.append((np.abs(ra.v - rb.v), ra.e + rb.e))
    a = np.stack([m.v for m in ms])
    e = np.stack([m.e for m in ms])
    axis = np.argmax(a, 0)
    raw = pick(ms, axis)
    a2 = a.copy()
    np.put_along_axis(a2, axis[None], -np.inf, 0)
    k2 = np.argmax(a2, 0)
    n, f = float(F32(near)), float(F32(far))
    sel = np.arange(len(axis))
    margins = [("t_min axis", raw.v - a2[k2, sel], e[axis, sel] + e[k2, sel]),
               ("t_min slab", np.stack([g[0] for g in gaps])[axis, sel], np.stack([g[1] for g in gaps])[axis, sel]),
               ("raw vs near", np.where(raw.v == n, np.inf, np.abs(raw.v - n)), np.where(raw.v == n, 0.0, raw.e)),
               ("raw vs far", np.abs(raw.v - f), raw.e)]
    t_min = where(raw.v < n, n, where(raw.v > f, f, raw))
    return dict(t_min=t_min, raw=raw, axis=axis, upper=np.stack(ups)[axis, sel], margins=margins, through=(raw.v >= n) & (raw.v <= f))


def sample_world_ref(rays, S, near, far, step, jitter, box):
    tm = world_tmin_ref(rays, box, near, far)
    rngv = V(np.arange(S, dtype=np.float64)[None, :])
    if jitter is not None:
        rngv = rngv + V(f64(jitter)[:, None])
    t = tm["t_min"].reshape(-1, 1) + float(F32(step)) * rngv
    p = _points(rays, t)
    inside, clear = _box_mask(p, box)
    return dict(xyz=_stack(p), z=t, valid=inside, clear=clear, margins=[], tmin=tm)


def _rays(r, N, kind, enter=True):
    if kind == "ndc":   # (o_z = -1, d_z = 2 would put the first and the last sample ON the z faces: that is the on-face set)
        return np.concatenate([r.uniform(-1.2, 1.2, (N, 2)), r.uniform(-0.98, -0.9, (N, 1)), r.uniform(-0.6, 0.6, (N, 2)),
                               r.uniform(1.7, 1.95, (N, 1))], -1).astype(F32)
    if kind == "contract":
        d = r.standard_normal((N, 3))
        return np.concatenate([r.uniform(-0.4, 0.4, (N, 3)), d / np.linalg.norm(d, axis=-1, keepdims=True)], -1).astype(F32)
    # world: of four rays one comes from outside the box and enters it (its first unjittered sample lies ON the entry face, so
    # `enter` is off for the short unjittered sets), two start inside it (raw < near), one looks away and misses it
    o = r.uniform(-1, 1, (N, 3))
    o *= 3.0 / np.linalg.norm(o, axis=-1, keepdims=True)
    tgt = r.uniform(-0.5, 0.5, (N, 3))
    i = np.arange(N)
    ins = (i % 4 == 1) | (i % 4 == 2) | ((i % 4 == 0) & (not enter))
    o[ins] = r.uniform(-0.5, 0.5, (N, 3))[ins]
    tgt[i % 4 == 3] = (2.0 * o + 0.3 * r.standard_normal((N, 3)))[i % 4 == 3]   # looks away from the box
    d = tgt - o
    return np.concatenate([o, d / np.linalg.norm(d, axis=-1, keepdims=True)], -1).astype(F32)


def sampler_case(kind, N, S, jit, far=None, seed=0):
    """kind ndc / contract / world; jit: jitter on"""
    def make(r):
        rays = _rays(r, N, kind, jit or S >= 64)
        if kind == "ndc":
            near, fr = 0.0, 1.0
            j = r.uniform(0, 1, S).astype(F32) if jit else None
            ref = sample_ndc_ref(rays, S, near, fr, j, BOX)
            return dict(kind=kind, rays=rays, S=S, near=near, far=fr, jitter=j, jout=None, box=BOX, ref=ref, margins=ref["margins"])
        if kind == "contract":
            near, fr = 0.05, float(far or 6.0)
            j = r.uniform(0, 1, S - S // 2 + 1).astype(F32) if jit else None
            jo = r.uniform(0, 1, S // 2 + 1).astype(F32) if jit else None
            ref = sample_contract_ref(rays, S, near, fr, j, jo)
            return dict(kind=kind, rays=rays, S=S, near=near, far=fr, jitter=j, jout=jo, box=None, ref=ref, margins=ref["margins"])
        near, fr, step = 0.5, 6.0, 0.0123
        j = r.uniform(0, 1, N).astype(F32) if jit else None
        ref = sample_world_ref(rays, S, near, fr, step, j, WBOX)
        return dict(kind=kind, rays=rays, S=S, near=near, far=fr, step=step, jitter=j, jout=None, box=WBOX, ref=ref,
                    margins=ref["margins"])
    return until_ok(make, 30, len(kind), N, S, int(jit), int(far or 0), seed)


def sampler_cases():
    out = []
    for kind in ("ndc", "contract", "world"):
        for S in SAMPLE_S:
            if S == 1 and kind == "contract":
                continue
            for jit in (False, True):
                for N in sorted({1, max(1, 255 // S), 256 // S + 1, 5}):   # N S on both sides of one 256-thread block
                    fars = (6.0, 256.0) if kind == "contract" else (None,)
                    for far in fars:
                        out.append((f"sample {kind} N={N} S={S} jitter={jit}" + (f" far={far}" if far else ""),
                                    dict(kind=kind, N=N, S=S, jit=jit, far=far)))
    return out


def on_face_case(kind):
    """points ON a face to the bit through exactly representable rays: valid must be 1.  ndc: S = 5, z = 0, 1/4 .. 1 exactly
    (near 0, far 1, no jitter), d a multiple of 4 in units of 2^-k so that o + d z is exact and equals hi / lo of a dyadic box.
    world: step 2^-6, near = raw exactly (the ray starts ON the entry face), march along one axis."""
    box = np.array([[-1.5, -1.75, -1.0], [1.5, 1.75, 1.0]], F32)
    if kind == "ndc":
        rays = np.array([[0.5, 0.25, -1.0, 1.0, 1.5, 2.0],      # z = 1: (1.5, 1.75, 1.0) == hi on all three axes
                         [-0.5, -0.75, -1.0, -1.0, -1.0, 0.0],  # z = 1: (-1.5, -1.75, -1) == lo
                         [1.5, 0.0, 1.0, 0.0, 0.5, 0.0],        # on hi.x and hi.z for every z
                         [1.5, 0.0, 0.0, 0.5, 0.0, 0.0]], F32)  # leaves through hi.x: on the face at z = 0 only
        expect = np.array([[1, 1, 1, 1, 1], [1, 1, 1, 1, 1], [1, 1, 1, 1, 1], [1, 0, 0, 0, 0]], bool)
        return dict(kind=kind, rays=rays, S=5, near=0.0, far=1.0, jitter=None, box=box, expect=expect)
    rays = np.array([[-3.5, 0.5, 0.25, 1.0, 0.0, 0.0],     # enters at x = lo.x = -1.5 (raw = 2): sample 0 ON the face
                     [3.5, 0.5, 0.25, -1.0, 0.0, 0.0],     # enters at hi.x
                     [0.5, 1.75, -1.0, 0.0, 0.0, 0.0]], F32)   # d == 0 on every axis, origin ON hi.y and lo.z: never moves
    S = 5
    expect = np.ones((3, S), bool)
    return dict(kind=kind, rays=rays, S=S, near=0.0, far=8.0, step=2.0 ** -6, jitter=None, box=box, expect=expect)


def contract_exact_case():
    """the contract sampler where float32 is exact: near 0, S = 8: the inner edges 0, 1/2, 1, 3/2, 2 and their midpoints 1/4, 3/4, 5/4,
    7/4 are dyadic, and so are the points of dyadic rays while they stay inside the unit cube (z < 1).  Compared bit for bit: a
    midpoint factor one ulp off 1/2 stays inside any rounding bound, not inside this."""
    rays = np.array([[0.0, 0.0, 0.0, 1.0, 0.5, -0.25], [0.125, -0.25, 0.5, -0.5, 0.25, 0.5]], F32)
    z = np.array([0.25, 0.75, 1.25, 1.75])
    pts = f64(rays)[:, None, :3] + f64(rays)[:, None, 3:] * z[None, :2, None]
    return dict(kind="contract", rays=rays, S=8, near=0.0, far=6.0, jitter=None, jout=None, box=None, z_inner=z, pts_inner=pts)


# ----------------------------------------------------------------------------------------------------------------------------
# Sampler adjoints (k_sample_bwd, k_sample_world_bwd)
# ----------------------------------------------------------------------------------------------------------------------------
def sample_bwd_ref(rays, z, contract, g_xyz, pre):
    """g_rays V [N,6] = pre + adjoint of xyz = (contract of) o + d z; z float32 [N,S] as the forward stored it"""
    N, S = z.shape
    t = V(f64(z))
    g = [V(f64(g_xyz)[:, :, k]) for k in range(3)]
    margins = []
    if contract:
        p = _points(rays, t)
        k, nrm, gap, eb = argmax3(p)
        big = nrm.v > 1.0
        safe = where(big, nrm, 1.0)
        n2 = safe * safe
        sc = 2.0 / safe - 1.0 / n2
        dsc = (-2.0 / n2 + 2.0 / (n2 * safe)).x2(1.0)
        sgn = np.where(pick(p, k).v > 0, 1.0, -1.0)
        gp = dot3(g, p)
        add = gp * V(dsc.v * sgn, dsc.e, dsc.r)
        g = [where(big, where(k == i, g[i] * sc + add, g[i] * sc), g[i]) for i in range(3)]
        margins = [("nrm > 1", np.abs(nrm.v - 1.0), nrm.e), ("arg-max", np.where(big, gap, np.inf), np.where(big, eb, 0.0))]
    depth = lane_depth(S)
    cols = [vsum(g[k], 1, depth) for k in range(3)] + [vsum(g[k] * t, 1, depth) for k in range(3)]
    out = [accumulate(f64(pre)[:, i], cols[i]) for i in range(6)]
    return dict(g_rays=_stack(out), margins=margins)


def sample_world_bwd_ref(rays, z, near, far, box, g_xyz, g_z, pre):
    N, S = z.shape
    t = V(f64(z))
    R = f64(rays)
    zero = V(np.zeros((N, S)))
    g = [V(f64(g_xyz)[:, :, k]) if g_xyz is not None else zero for k in range(3)]
    depth = lane_depth(S)
    go = [vsum(g[k], 1, depth) for k in range(3)]
    gd = [vsum(g[k] * t, 1, depth) for k in range(3)]
    terms = [g[k] * V(R[:, 3 + k, None]) for k in range(3)] + ([V(f64(g_z))] if g_z is not None else [])
    gt = vsum(V(np.stack([x.v for x in terms], -1).reshape(N, -1), np.stack([x.e for x in terms], -1).reshape(N, -1)), 1, depth + 3)
    tm = world_tmin_ref(rays, box, near, far)
    ax, thr = tm["axis"], tm["through"]
    sel = np.arange(N)
    dax = R[sel, 3 + ax]
    vec = V(np.where(dax == 0.0, eps6(), dax))
    a_o = gt * (-1.0 / vec)
    a_d = gt * (-tm["raw"] / vec)
    for k in range(3):
        go[k] = where(thr & (ax == k), go[k] + a_o, go[k])
        gd[k] = where(thr & (ax == k) & (dax != 0.0), gd[k] + a_d, gd[k])
    out = [accumulate(f64(pre)[:, i], (go + gd)[i]) for i in range(6)]
    return dict(g_rays=_stack(out), margins=tm["margins"], tmin=tm)


def sample_bwd_case(kind, N, S, seed=0):
    """kind "ndc" / "contract": rays whose samples lie on both sides of nrm = 1 with the arg-max on every axis and sign"""
    def make(r):
        rays = _rays(r, N, kind)
        if kind == "contract":   # row n: the dominant direction component is axis n % 3, sign by (n // 3) % 2
            for n in range(N):
                d = 0.3 * r.uniform(-1, 1, 3)
                d[n % 3] = 1.0 if (n // 3) % 2 == 0 else -1.0
                rays[n, 3:] = (d / np.linalg.norm(d)).astype(F32)
                rays[n, :3] = r.uniform(-0.2, 0.2, 3).astype(F32)
            z = contract_t_ref(max(S, 2), 0.05, 6.0, None, None).v[:S]
            z = np.tile(z * r.uniform(0.9, 1.1, (N, 1)), (1, 1)).astype(F32)
        else:
            z = np.tile(np.sort(r.uniform(0, 1, S)), (N, 1)).astype(F32)
        g = r.standard_normal((N, S, 3)).astype(F32)
        pre = r.standard_normal((N, 6)).astype(F32)
        ref = sample_bwd_ref(rays, z, kind == "contract", g, pre)
        return dict(kind=kind, rays=rays, z=z, g=g, pre=pre, ref=ref, margins=ref["margins"])
    return until_ok(make, 40, len(kind), N, S, seed)


WORLD_BWD_ROWS = ("x lower", "x upper", "y lower", "y upper", "z lower", "z upper", "raw < near", "raw > far", "raw == near",
                  "d_x == 0", "d_y == 0", "d_z == 0")


def sample_world_bwd_case(S, g_mode="both", seed=0):
    """one ray per WORLD_BWD_ROWS entry (N = 12), box WBOX, near 0.5, far 6.  "raw == near": an axis-aligned ray from a dyadic
    origin whose entry depth is exactly 0.5.  "d_k == 0": the origin lies outside the slab of axis k on the far side of its lower
    bound, so that the 1e-6 quotient of that axis is the largest and is selected (its depth is clamped by far = 1e7 there)."""
    def make(r):
        lo, hi = f64(WBOX)[0], f64(WBOX)[1]
        rows, nears, fars = [], [], []
        for name in WORLD_BWD_ROWS:
            o, d = r.uniform(-0.3, 0.3, 3) * (hi - lo) / 2, None
            if name[2:] in ("lower", "upper"):
                k = "xyz".index(name[0])
                tgt = r.uniform(-0.3, 0.3, 3) * (hi - lo) / 2
                o = tgt.copy()
                o[k] = (lo[k] - 2.0) if name.endswith("lower") else (hi[k] + 2.0)
                d = tgt - o
            elif name == "raw < near":
                d = r.standard_normal(3)
            elif name == "raw > far":
                o = np.array([-9.0, 0.1, 0.05])
                d = np.array([1.0, 0.01, 0.02])
            elif name == "raw == near":
                o, d = np.array([-1.5, 0.25, 0.125]), np.array([1.0, 0.0, 0.0])
            else:
                k = "xyz".index(name[2])
                o = r.uniform(-0.2, 0.2, 3)
                o[k] = lo[k] - 0.5
                d = r.uniform(0.3, 1.0, 3) * np.sign(r.standard_normal(3))
                d[k] = 0.0
            if name != "raw == near":
                d = d / np.linalg.norm(d)
            rows.append(np.r_[o, d])
        rays = np.array(rows, F32)
        N = len(rows)
        near, far = 0.5, 6.0
        z = (r.uniform(0.5, 6.0, (N, 1)) + 0.0123 * np.arange(S)[None, :]).astype(F32)
        g = r.standard_normal((N, S, 3)).astype(F32) if g_mode in ("both", "xyz") else None
        gz = r.standard_normal((N, S)).astype(F32) if g_mode in ("both", "z") else None
        pre = r.standard_normal((N, 6)).astype(F32)
        ref = sample_world_bwd_ref(rays, z, near, far, WBOX, g, gz, pre)
        return dict(rays=rays, z=z, near=near, far=far, box=WBOX, g=g, gz=gz, pre=pre, ref=ref, margins=ref["margins"])
    return until_ok(make, 41, S, len(g_mode), seed)


def sample_world_bwd_zero_case(S, seed=0):
    """d_k == 0 with the 1e-6 quotient SELECTED and inside [near, far]: far = 1e7.  o_k = lo_k - 0.5: (lo_k - o_k) / 1e-6 = 5e5"""
    c = sample_world_bwd_case(S, "both", seed)
    rays = c["rays"][9:12].copy()
    z, g, gz, pre = c["z"][9:12], c["g"][9:12], c["gz"][9:12], c["pre"][9:12]
    ref = sample_world_bwd_ref(rays, z, 0.5, 1e7, WBOX, g, gz, pre)
    return dict(rays=rays, z=z, near=0.5, far=1e7, box=WBOX, g=g, gz=gz, pre=pre, ref=ref, margins=ref["margins"])


# ----------------------------------------------------------------------------------------------------------------------------
# Induced flow (flow_ray_seed / flow_ray_fwd, k_induce_flow, k_induce_flow_bwd)
# ----------------------------------------------------------------------------------------------------------------------------
IFB_WAVES = 8
FLOW_N = (1, 7, 8, 9, 17)
FLOW_S = (1, 63, 64, 65, 130)
FLOW_OUTS = ("g_weights", "g_pts", "g_rays", "g_c2w", "g_focal")


def flow_seed_ref(w, pts, rays, contract):
    """P = sum w p + (1 - acc) far -> dict(P, far, acc, f0, fk, fn, fs, fbig, margins)"""
    N, S = w.shape
    depth = lane_depth(S)
    wv = V(f64(w))
    acc = vsum(wv, 1, depth)
    ps = [vsum(wv * V(f64(pts)[:, :, k]), 1, depth + 1) for k in range(3)]   # (+ 1: an unfused product rounds before the sum)
    R = f64(rays)
    o, d = [V(R[:, k]) for k in range(3)], [V(R[:, 3 + k]) for k in range(3)]
    res = dict(acc=acc, ps=ps, margins=[])
    if not contract:
        far = [o[k] + d[k] for k in range(3)]
    else:
        f0 = [o[k] + d[k].x2(256.0) for k in range(3)]
        fk, fn, gap, eb = argmax3(f0)
        fbig = fn.v > 1.0
        safe = where(fbig, fn, 1.0)
        fs = 2.0 - 1.0 / safe
        far = [where(fbig, fs * (f0[k] / safe), f0[k]) for k in range(3)]
        res.update(f0=f0, fk=fk, fn=safe, fs=fs, fbig=fbig)
        res["margins"] += [("far nrm > 1", np.abs(fn.v - 1.0), fn.e), ("far arg-max", np.where(fbig, gap, np.inf), np.where(fbig, eb, 0.0))]
    one_acc = 1.0 - acc
    res.update(far=far, one_acc=one_acc, P=[ps[k] + one_acc * far[k] for k in range(3)])
    return res


def flow_ref(H, W, focal, c2w, w, pts, p2d, rays, contract, g_flow=None, g_disp=None, pre=None, want_bwd=True):
    """-> dict(flow V [N,2], disp V [N], world, cam2, margins; g_weights, g_pts, g_rays, g_c2w, g_focal V with `pre` added)"""
    N, S = w.shape
    f = V(float(F32(focal)))
    s = flow_seed_ref(w, pts, rays, contract)
    P, margins = s["P"], list(s["margins"])
    M = f64(c2w).reshape(N, 12)
    if not contract:
        inside = (P[2].v >= -1.0) & (P[2].v <= clamp_hi())
        c = where(P[2].v < -1.0, -1.0, where(P[2].v > clamp_hi(), clamp_hi(), P[2]))
        margins.append(("P.z clamp", np.minimum(np.abs(P[2].v + 1.0), np.abs(P[2].v - clamp_hi())), P[2].e))
        cm1 = c - 1.0
        pz = 2.0 / cm1
        world = [(-P[0] * pz * float(W)).x2(0.5) / f, (-P[1] * pz * float(H)).x2(0.5) / f, pz]
    else:
        wk, wn, gap, eb = argmax3(P)
        wbig = wn.v > 1.0
        m = where(wbig, wn, 1.5)
        wsc = -(1.0 / (m - 2.0))
        world = [where(wbig, P[k] / m * wsc, P[k]) for k in range(3)]
        margins += [("wn > 1", np.abs(wn.v - 1.0), wn.e), ("world arg-max", np.where(wbig, gap, np.inf), np.where(wbig, eb, 0.0))]
    q = [world[j] - V(M[:, j * 4 + 3]) for j in range(3)]
    cam = [(q[0] * V(M[:, 0 + i]) + q[1] * V(M[:, 4 + i])) + q[2] * V(M[:, 8 + i]) for i in range(3)]
    u = cam[0] / (-cam[2]) * f + float(W) * 0.5
    v = -cam[1] / (-cam[2]) * f + float(H) * 0.5
    disp = 1.0 + 2.0 / cam[2]
    P2d = f64(p2d)
    res = dict(flow=_stack([u - V(P2d[:, 0]), v - V(P2d[:, 1])]), disp=disp, cam2=cam[2], margins=margins, world=world, P=P,
               acc=s["acc"])
    if not want_bwd:
        return res
    zero = V(np.zeros(N))
    gu, gv = (V(f64(g_flow)[:, 0]), V(f64(g_flow)[:, 1])) if g_flow is not None else (zero, zero)
    gd = V(f64(g_disp).reshape(N)) if g_disp is not None else zero
    ic2 = 1.0 / cam[2]
    gcam = [-gu * f * ic2, gv * f * ic2, (gu * cam[0] - gv * cam[1]) * f * ic2 * ic2 - gd.x2(2.0) * ic2 * ic2]
    gf = -gu * cam[0] * ic2 + gv * cam[1] * ic2
    gq = [(gcam[0] * V(M[:, j * 4 + 0]) + gcam[1] * V(M[:, j * 4 + 1])) + gcam[2] * V(M[:, j * 4 + 2]) for j in range(3)]
    gM = [None] * 12
    for j in range(3):
        for i in range(3):
            gM[j * 4 + i] = q[j] * gcam[i]
        gM[j * 4 + 3] = -gq[j]
    if not contract:
        sx, sy = V(float(W) / 2.0) / f, V(float(H) / 2.0) / f
        gpz = (-gq[0] * P[0] * sx - gq[1] * P[1] * sy) + gq[2]
        gf = gf + (-((world[0] * gq[0] + world[1] * gq[1]) / f))
        gc = gpz * (-2.0 / (cm1 * cm1))
        gP = [-gq[0] * pz * sx, -gq[1] * pz * sy, where(inside, gc, 0.0)]
        res["clamped"] = ~inside
    else:
        sc = wsc / m
        mm = m * (2.0 - m)
        ds = (m.x2(2.0) - 2.0) / (mm * mm)
        dot = dot3(gq, P)
        sgn = np.where(pick(P, wk).v >= 0, 1.0, -1.0)
        add = dot * ds * V(sgn)
        gP = [where(wbig, where(wk == i, gq[i] * sc + add, gq[i] * sc), gq[i]) for i in range(3)]
    far = s["far"]
    gacc = -dot3(gP, far)
    pv = [V(f64(pts)[:, :, k]) for k in range(3)]
    col = lambda x: x.reshape(N, 1)
    gw = ((col(gP[0]) * pv[0] + col(gP[1]) * pv[1]) + col(gP[2]) * pv[2]) + col(gacc)
    wv = V(f64(w))
    gpts = _stack([wv * col(gP[k]) for k in range(3)])
    gfar = [s["one_acc"] * gP[k] for k in range(3)]
    if not contract:
        gr = gfar + gfar
    else:
        nn, fk, f0 = s["fn"], s["fk"], s["f0"]
        gsc = s["fs"] / nn
        dotf = dot3(gfar, f0)
        sgn = np.where(pick(f0, fk).v >= 0, 1.0, -1.0)
        add = dotf * (2.0 - nn.x2(2.0)) / (nn * nn * nn) * V(sgn)
        g0 = [where(s["fbig"], where(fk == i, gfar[i] * gsc + add, gfar[i] * gsc), gfar[i]) for i in range(3)]
        gr = g0 + [x.x2(256.0) for x in g0]
    pre = pre or {}
    z = lambda name, shape: f64(pre[name]).reshape(shape) if pre.get(name) is not None else np.zeros(shape)
    res["g_weights"] = accumulate(z("g_weights", (N, S)), gw)
    res["g_pts"] = accumulate(z("g_pts", (N, S, 3)), gpts)
    res["g_rays"] = accumulate(z("g_rays", (N, 6)), _stack(gr))
    res["g_c2w"] = accumulate(z("g_c2w", (N, 12)), _stack(gM))
    res["g_focal"] = scatter_sum(gf, np.zeros(N, np.int64), 1, z("g_focal", (1,)))
    res["gP"] = gP
    return res


def _rotations(r, N):
    q, _ = np.linalg.qr(r.standard_normal((N, 3, 3)))
    return q


FLOW_ROWS_NDC = ("plain", "zero weights", "unit weights", "P.z < -1", "P.z > 1 - 1e-6")
FLOW_ROWS_CONTRACT = ("plain", "zero weights", "unit weights", "wn <= 1", "zero direction")


def flow_case(contract, N, S, seed=0, singular=False):
    """row n takes regime n % 5 of FLOW_ROWS_*.  The camera translation is solved (float64, then rounded) so that the point lands
    at a chosen camera-space position: |cam_z| in [0.5, 3] of the point's own scale, both signs -- or, `singular`, log-uniform from
    1 down to 2^-19.5 (ndc) / 2^-14.5 (contract) of it."""
    rows = FLOW_ROWS_CONTRACT if contract else FLOW_ROWS_NDC

    def make(r):
        H, W = 24, 40
        focal = F32(0.5 * max(H, W) * 1.7320508)
        lim = 1.9 if contract else 0.9
        w = r.uniform(0, 1, (N, S))
        w = w / w.sum(-1, keepdims=True) * r.uniform(0.2, 0.8, (N, 1))
        pts = r.uniform(-lim, lim, (N, S, 3))
        if contract:
            d = r.standard_normal((N, 3))
            rays = np.concatenate([r.uniform(-0.2, 0.2, (N, 3)), d / np.linalg.norm(d, axis=-1, keepdims=True)], -1)
        else:
            rays = np.concatenate([r.uniform(-0.8, 0.8, (N, 2)), -np.ones((N, 1)), r.uniform(-0.1, 0.1, (N, 2)), 2 * np.ones((N, 1))], -1)
        for n in range(N):
            kind = rows[n % 5]
            if kind == "zero weights":
                w[n] = 0
            elif kind == "unit weights":
                w[n] = w[n] / w[n].sum()
            elif kind == "P.z < -1":
                pts[n, :, 2] = r.uniform(-3.0, -2.0, S)
                w[n] = w[n] / w[n].sum() * 0.9
                rays[n, 2], rays[n, 5] = -1.0, 0.0
            elif kind == "P.z > 1 - 1e-6":
                pts[n, :, 2] = r.uniform(1.5, 2.0, S)
                w[n] = w[n] / w[n].sum() * 0.9
            elif kind == "plain" and contract:   # a cluster outside the unit cube: wn > 1
                ctr = r.uniform(-1.0, 1.0, 3)
                ctr[r.integers(0, 3)] = r.uniform(1.3, 1.8) * np.sign(r.standard_normal())
                pts[n] = ctr + 0.1 * r.uniform(-1, 1, (S, 3))
                w[n] = w[n] / w[n].sum() * 0.9
            elif kind == "wn <= 1":
                pts[n] *= 0.2
                w[n] = w[n] / w[n].sum()
            elif kind == "zero direction":
                rays[n, 3:] = 0
                rays[n, :3] = r.uniform(-0.6, 0.6, 3)
        w, pts, rays = w.astype(F32), pts.astype(F32), rays.astype(F32)
        R = _rotations(r, N)
        c2w = np.concatenate([R, np.zeros((N, 3, 1))], -1).astype(F32)
        fw = flow_ref(H, W, focal, c2w, w, pts, np.zeros((N, 2), F32), rays, contract, want_bwd=False)
        world = np.stack([x.v for x in fw["world"]], -1)
        scale = np.maximum(1.0, np.abs(world).max(-1))
        cz = 2.0 ** r.uniform(-14.5 if contract else -19.5, 0, N) if singular else r.uniform(0.5, 3.0, N)
        cam = np.stack([r.uniform(-1, 1, N), r.uniform(-1, 1, N), cz * np.sign(r.standard_normal(N))], -1) * scale[:, None]
        c2w[:, :, 3] = (world - np.einsum("nji,ni->nj", f64(c2w[:, :, :3]), cam)).astype(F32)
        p2d = r.uniform(0, 40, (N, 2)).astype(F32)
        g_flow, g_disp = r.standard_normal((N, 2)).astype(F32), r.standard_normal(N).astype(F32)
        pre = dict(g_weights=r.standard_normal((N, S)).astype(F32), g_pts=r.standard_normal((N, S, 3)).astype(F32),
                   g_rays=r.standard_normal((N, 6)).astype(F32), g_c2w=r.standard_normal((N, 12)).astype(F32),
                   g_focal=r.standard_normal(1).astype(F32))
        ref = flow_ref(H, W, focal, c2w, w, pts, p2d, rays, contract, g_flow, g_disp, pre)
        rho = max(ref[k].r.max() for k in ("flow", "disp") + FLOW_OUTS)
        m = list(ref["margins"])
        if not singular:
            m.append(("divisor bounds", RHO_ORDINARY * np.ones(1), rho / SECOND * np.ones(1)))
        return dict(contract=contract, H=H, W=W, focal=focal, c2w=c2w, w=w, pts=pts, p2d=p2d, rays=rays, g_flow=g_flow,
                    g_disp=g_disp, pre=pre, ref=ref, margins=m, rows=[rows[n % 5] for n in range(N)])
    return until_ok(make, 50, int(contract), N, S, int(singular), seed)


def flow_cases():
    out = []
    for contract in (False, True):
        for N in FLOW_N:
            out.append(dict(contract=contract, N=N, S=65))
        for S in FLOW_S:
            out.append(dict(contract=contract, N=17, S=S))
    return [(f"flow {'contract' if k['contract'] else 'ndc'} N={k['N']} S={k['S']}", k) for k in out]
