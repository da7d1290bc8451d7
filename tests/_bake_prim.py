"""Float64 reference of the texture atlas (csrc/rdrf_bake.hip; include/rodynrf.h, rdrf_bake_texels): layout, ownership,
barycentric weights, texel points, face normals, texture coordinates, the footprint of a bilinear fetch, and the error bounds
of the kernel's fp32 evaluation, counted from its operations.

The atlas: squares of q x q texels, R = Wt // q to a row; square s = f >> 1 at ((s % R) q, (s // R) q) holds face 2s where
i + j <= q - 1 and face 2s + 1 elsewhere ((i, j): the texel's indices inside the square).  A texel's weights are those of its
centre (i + 0.5, j + 0.5) against the face's local corners

    lower  (0.5, 0.5), (q - 1.5, 0.5), (0.5, q - 1.5)      w1 = i / (q - 2),           w2 = j / (q - 2)
    upper  (q - 0.5, q - 0.5), (2.5, q - 0.5), (q - 0.5, 2.5)   w1 = (q - 1 - i) / (q - 3),   w2 = (q - 1 - j) / (q - 3)

and w0 = 1 - w1 - w2, which is negative on the two diagonals i + j = q - 1 and i + j = q: the gutters.

The bound of a texel point.  The kernel evaluates, with one rounding per operation (u = 2^-24) and exact conversions of the
small integers,  w1 = fl(a / d), w2 = fl(b / d), w0 = fl(fl(1 - w1) - w2), p = fl(fl(fl(w0 v0) + fl(w1 v1)) + fl(w2 v2)).
To first order  |dw1| <= u |w1|, |dw2| <= u |w2| (the two divisions) and
|dw0| <= u (|w1| + |1 - w1| + |w2| + |w0|)  (both divisions, both subtractions), so per coordinate

    |dp| <= |dw0| |v0| + u |w1 v1| + u |w2 v2|                    the weights
          + u (|w0 v0| + |w1 v1| + |w2 v2|)                       the three products
          + u (|w0 v0| + |w1 v1|) + u (|w0 v0| + |w1 v1| + |w2 v2|)   the two additions
        = u [ (5 |w0| + c) |v0| + 4 |w1 v1| + 3 |w2 v2| ],   c = |w1| + |1 - w1| + |w2| - |w0| >= 0
       <= 5 u (|w0| |v0| + |w1| |v1| + |w2| |v2|) + u c |v0|.

The first term is k u (|w0||v0| + |w1||v1| + |w2||v2|) with k = 5.  The second is what w0 = 1 - w1 - w2 costs where it
cancels: on the edge opposite v0 the exact w0 is 0 while the computed one is a rounding error of the divisions (q = 5, texel
(1, 2): fl(1/3) and fl(2/3) leave w0 = 2^-25 or so), so no multiple of |w0| |v0| bounds the error there -- take v1 = v2 = 0.
Inside the triangle (all weights >= 0) c = w1 + 2 w2: the errors of the divisions and of 1 - w1 that w0 inherits, carried by
|v0|; it is counted from the operations like the rest, not a slack factor.  POINT_SLACK = 1 / (1 - 8 u) covers the second-order terms, and three units
of the smallest subnormal the underflow of the products.

Away from the cancellation the short form does hold, with a larger k: where c <= 3 |w0| the bound above is at most
8 u (|w0||v0| + |w1||v1| + |w2||v2|)  (SHORT_K = 5 + 3).  The tests assert that form too on those texels (the corner v0 and
the texels around it), so the term in c cannot cover for an error where nothing cancels.

The bound of a face's view direction  d = -n / |n|, n = (v1 - v0) x (v2 - v0):  e = fl(v_k - v0) (u each),
l = fl(e1a e2b), r = fl(e1b e2a), n_c = fl(l - r): |dn_c| <= 4 u A_c with A_c = |e1a e2b| + |e1b e2a|; n2 = three squares and
two additions of positive terms (3 u relative), the root (u, on top of half of n2's) and the division (u): 3.5 u relative on
d_c.  With |n^_c| / |n^| <= 1:  |dd_c| <= (|dn_c| + |dn|_2) / |n| + 3.5 u.  NORMAL_SLACK = 1 / (1 - 16 u).
"""
import numpy as np

U = 2.0 ** -24
POINT_K = 5
SHORT_K = 8
POINT_SLACK = 1.0 / (1.0 - 8 * U)
NORMAL_SLACK = 1.0 / (1.0 - 16 * U)
TINY = 3 * 2.0 ** -149


def layout(F, q, width=None):
    """(Wt, Ht, R); width=None: the smallest power of two >= q ceil(sqrt(ceil(F / 2)))"""
    nsq = (F + 1) // 2
    if width is None:
        side = int(np.ceil(np.sqrt(nsq)))
        while side * side < nsq:
            side += 1
        while side > 0 and (side - 1) * (side - 1) >= nsq:
            side -= 1
        need = q * max(1, side)
        Wt = 1
        while Wt < need:
            Wt *= 2
    else:
        Wt = width
    R = Wt // q
    return Wt, q * ((nsq + R - 1) // R), R


def ownership(F, q, Wt, Ht=None):
    """dict(face [Ht,Wt] (-1: none), upper [Ht,Wt] bool, i, j [Ht,Wt]) by the rules of the issue, texel by texel"""
    _, H0, R = layout(F, q, Wt)
    Ht = H0 if Ht is None else Ht
    y, x = np.meshgrid(np.arange(Ht), np.arange(Wt), indexing="ij")
    i, j = x % q, y % q
    s = (y // q) * R + x // q
    upper = i + j > q - 1
    f = 2 * s + upper
    face = np.where((x < R * q) & (f < F), f, -1)
    return {"face": face.astype(np.int64), "upper": upper, "i": i, "j": j}


def weights(q, i, j, upper, dtype=np.float64):
    """(w0, w1, w2) in `dtype`, in the kernel's order: two divisions, w0 = (1 - w1) - w2"""
    t = dtype
    a = np.where(upper, q - 1 - i, i).astype(t)
    b = np.where(upper, q - 1 - j, j).astype(t)
    d = np.where(upper, q - 3, q - 2).astype(t)
    w1 = (a / d).astype(t)
    w2 = (b / d).astype(t)
    w0 = ((t(1.0) - w1).astype(t) - w2).astype(t)
    return w0, w1, w2


def points(verts, faces, q, Wt, Ht=None, dtype=np.float64):
    """dict(points [Ht,Wt,3] in `dtype`, bound [Ht,Wt,3] (float64), face, issue_form: the bound's first term alone,
    short_ok / short_form: the texels where c <= 3 |w0| and the short form with SHORT_K there): dtype=float32 is the kernel's evaluation, operation
    by operation; unowned texels get the point 0"""
    F = len(faces)
    own = ownership(F, q, Wt, Ht)
    face, t = own["face"], dtype
    v = np.asarray(verts, dtype=np.float32).astype(t)
    fv = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    safe = np.where(face >= 0, face, 0)
    corner = [v[fv[safe, k]] if F else np.zeros(face.shape + (3,), dtype=t) for k in range(3)]
    w0, w1, w2 = weights(q, own["i"], own["j"], own["upper"], t)
    a0, a1, a2 = ((w[..., None] * c).astype(t) for w, c in zip((w0, w1, w2), corner))
    p = ((a0 + a1).astype(t) + a2).astype(t)
    e0, e1, e2 = (np.abs(w.astype(np.float64)) for w in (w0, w1, w2))
    c0, c1, c2 = (np.abs(c.astype(np.float64)) for c in corner)
    issue_sum = e0[..., None] * c0 + e1[..., None] * c1 + e2[..., None] * c2
    c = e1 + np.abs(1.0 - w1.astype(np.float64)) + e2 - e0
    cancel = c[..., None] * c0
    bound = POINT_SLACK * U * (POINT_K * issue_sum + cancel) + TINY
    owned = (face >= 0)[..., None]
    return {"points": np.where(owned, p, t(0.0)), "bound": np.where(owned, bound, 0.0), "face": face,
            "issue_form": np.where(owned, POINT_K * U * issue_sum, 0.0),
            "short_ok": (face >= 0) & (c <= 3.0 * e0), "short_form": POINT_SLACK * U * SHORT_K * issue_sum + TINY}


def face_dirs(verts, faces):
    """(d [F,3], bound [F,3], ok [F]): d = -n / |n| of every face in float64, n = (v1 - v0) x (v2 - v0); ok is false where
    n . n is 0 or not finite (the kernel hands (0, 0, 1) to such a face)"""
    v = np.asarray(verts, dtype=np.float32).astype(np.float64)
    fv = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    v0, v1, v2 = v[fv[:, 0]], v[fv[:, 1]], v[fv[:, 2]]
    e1, e2 = v1 - v0, v2 - v0
    with np.errstate(all="ignore"):
        n = np.cross(e1, e2)
        A = np.stack([np.abs(e1[:, (c + 1) % 3] * e2[:, (c + 2) % 3]) + np.abs(e1[:, (c + 2) % 3] * e2[:, (c + 1) % 3]) for c in range(3)], -1)
        n2 = (n * n).sum(-1)
        ok = np.isfinite(n2) & (n2 > 0)
        length = np.sqrt(np.where(ok, n2, 1.0))[:, None]
        d = np.where(ok[:, None], -n / length, np.array([0.0, 0.0, 1.0]))
        dn = 4 * U * A
        bound = NORMAL_SLACK * ((dn + np.sqrt((dn * dn).sum(-1))[:, None]) / length + 3.5 * U)
    return d, np.where(ok[:, None], bound, 0.0), ok


def local_corners(q, upper):
    """the three local UV corners of a face, in texel units, in the order v0, v1, v2"""
    if upper:
        return np.array([[q - 0.5, q - 0.5], [2.5, q - 0.5], [q - 0.5, 2.5]])
    return np.array([[0.5, 0.5], [q - 1.5, 0.5], [0.5, q - 1.5]])


def corners_texel(F, q, Wt):
    """[F,3,2] float64: the corners in atlas texel units (exact: half-integers)"""
    _, _, R = layout(F, q, Wt)
    out = np.zeros((F, 3, 2))
    for f in range(F):
        s = f >> 1
        out[f] = np.array([(s % R) * q, (s // R) * q], dtype=np.float64) + local_corners(q, bool(f & 1))
    return out


def uv(F, q, width=None):
    """[F,3,2] float64: ((sx + u) / Wt, (sy + v) / Ht)"""
    Wt, Ht, _ = layout(F, q, width)
    return corners_texel(F, q, Wt) / np.array([Wt, max(Ht, 1)], dtype=np.float64)


def footprint(px, py):
    """the texels (x, y) a bilinear fetch at the atlas position (px, py) -- texel units, texel (x, y) centred at
    (x + 0.5, y + 0.5) -- reads with a weight that is not zero"""
    out = []
    fx, fy = px - 0.5, py - 0.5
    x0, y0 = int(np.floor(fx)), int(np.floor(fy))
    for y, wy in ((y0, 1.0 - (fy - y0)), (y0 + 1, fy - y0)):
        for x, wx in ((x0, 1.0 - (fx - x0)), (x0 + 1, fx - x0)):
            if wx * wy != 0.0:
                out.append((x, y))
    return out


def bilinear(texture, px, py):
    """the bilinear fetch itself, float64, from a [Ht,Wt,C] array at atlas positions px, py (arrays, texel units); reads are
    clamped to the array (a fetch inside a triangle never needs the clamp)"""
    tex = np.asarray(texture, dtype=np.float64)
    fx, fy = np.asarray(px) - 0.5, np.asarray(py) - 0.5
    x0, y0 = np.floor(fx).astype(np.int64), np.floor(fy).astype(np.int64)
    ax, ay = (fx - x0)[..., None], (fy - y0)[..., None]
    cx = lambda x: np.clip(x, 0, tex.shape[1] - 1)
    cy = lambda y: np.clip(y, 0, tex.shape[0] - 1)
    return ((1 - ay) * ((1 - ax) * tex[cy(y0), cx(x0)] + ax * tex[cy(y0), cx(x0 + 1)])
            + ay * ((1 - ax) * tex[cy(y0 + 1), cx(x0)] + ax * tex[cy(y0 + 1), cx(x0 + 1)]))
