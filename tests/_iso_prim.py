"""Marching tetrahedra on the Kuhn split, restated in plain numpy float64 from the rules of DESIGN.md (section "Isosurface
meshes") -- not a port of csrc/rdrf_iso.hip: it loops over cubes, tetrahedra and edges, keeps a dict from (point, kind) to a
vertex, decides every winding geometrically, and applies the same ordering rules.  The property helpers of the mesh tests
(edge uses, orientation, Euler characteristic, signed volume) live here too.

Conventions (the ones the kernel and the tests must share):
  point linear index   (i * G1 + j) * G2 + k
  corner code          dx * 4 + dy * 2 + dz of a cube corner (0 .. 7)
  edge kind            corner code of (upper end - lower end) minus 1: 0 z, 1 y, 2 yz, 3 x, 4 xz, 5 xy, 6 xyz
  tetrahedron q        corners 0, bit(a), bit(a) | bit(b), 7 for (a, b, c) = PERMS[q], bit(axis) = 4 >> axis
  triangles of a tetrahedron with local corners 0 .. 3 (e(p, q) = the vertex on the edge between corners p and q):
     one corner u apart from the other three w1 < w2 < w3 (u alone inside or alone outside):  e(u,w1) e(u,w2) e(u,w3)
     two inside p < q, two outside r < s:  e(p,r) e(p,s) e(q,s)   then   e(p,r) e(q,s) e(q,r)
     each with its last two entries swapped where (b - a) x (c - a) would otherwise point at the inside corners."""
import itertools

import numpy as np

PERMS = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]
KIND_OFFSETS = [((c >> 2) & 1, (c >> 1) & 1, c & 1) for c in range(1, 8)]   # kind -> (dx, dy, dz)


def corner_offset(code):
    return np.array([(code >> 2) & 1, (code >> 1) & 1, code & 1])


def tet_corner_codes(q):
    a, b, _ = PERMS[q]
    return [0, 4 >> a, (4 >> a) | (4 >> b), 7]


_tri_memo = {}


def tet_triangles(codes, inside):
    """memo of _tet_triangles: 6 tetrahedra x 16 masks"""
    key = (tuple(codes), tuple(bool(b) for b in inside))
    if key not in _tri_memo:
        _tri_memo[key] = _tet_triangles(codes, inside)
    return _tri_memo[key]


def _tet_triangles(codes, inside):
    """the triangles of one tetrahedron as triples of local edges (p, q), p < q; wound by geometry on the unit cube with the
    vertices at the edge midpoints (the winding cannot change while every t stays inside (0, 1))"""
    ins = [i for i in range(4) if inside[i]]
    outs = [i for i in range(4) if not inside[i]]
    if not ins or not outs:
        return []
    if len(ins) == 1 or len(outs) == 1:
        u = ins[0] if len(ins) == 1 else outs[0]
        w = [i for i in range(4) if i != u]
        tris = [[(u, w[0]), (u, w[1]), (u, w[2])]]
    else:
        (p, q), (r, s) = ins, outs
        tris = [[(p, r), (p, s), (q, s)], [(p, r), (q, s), (q, r)]]
    P = [corner_offset(c).astype(np.float64) for c in codes]
    towards_outside = np.mean([P[i] for i in outs], 0) - np.mean([P[i] for i in ins], 0)
    out = []
    for tri in tris:
        m = [(P[a] + P[b]) / 2 for a, b in tri]
        n = np.cross(m[1] - m[0], m[2] - m[0])
        d = float(n @ towards_outside)
        assert d != 0.0
        if d < 0:
            tri = [tri[0], tri[2], tri[1]]
        out.append([(min(a, b), max(a, b)) for a, b in tri])
    return out


def lattice_positions(shape, aabb):
    aabb = np.asarray(aabb, dtype=np.float64).reshape(2, 3)
    return [aabb[0, d] + np.arange(shape[d], dtype=np.float64) / (shape[d] - 1) * (aabb[1, d] - aabb[0, d]) for d in range(3)]


def gradient(v, idx, spacing):
    """-grad v at a lattice point: central differences, one-sided at the boundary"""
    g = np.zeros(3)
    for d in range(3):
        lo, hi = list(idx), list(idx)
        lo[d] = max(idx[d] - 1, 0)
        hi[d] = min(idx[d] + 1, v.shape[d] - 1)
        g[d] = -(v[tuple(hi)] - v[tuple(lo)]) / ((hi[d] - lo[d]) * spacing[d])
    return g


def marching_tets(vol, level, aabb, flip=False, normals=False):
    """-> dict(verts [nv,3] f64, faces [nf,3] int64, keys [nv,2] (point, kind), t [nv], ends [nv,2,3] (outside, inside lattice
    index), normals [nv,3] + gnorm, gscale [nv] when asked).  vol: [G0,G1,G2] of any float type, used as float64."""
    v = np.asarray(vol, dtype=np.float64)
    G0, G1, G2 = v.shape
    level = float(level)
    inside = v >= level
    pos = lattice_positions(v.shape, aabb)
    spacing = [(pos[d][-1] - pos[d][0]) / (v.shape[d] - 1) for d in range(3)]
    lin = lambda i, j, k: (i * G1 + j) * G2 + k
    # vertices: every crossed edge, ascending (point, kind)
    keys, verts, ts, ends, nrm, gn, gs = [], [], [], [], [], [], []
    index = {}
    mixed = np.zeros((G0, G1, G2), dtype=bool)   # points that own a crossed edge
    for kind, (dx, dy, dz) in enumerate(KIND_OFFSETS):
        a = inside[:G0 - dx, :G1 - dy, :G2 - dz]
        b = inside[dx:, dy:, dz:]
        mixed[:G0 - dx, :G1 - dy, :G2 - dz] |= a != b
    for i, j, k in np.argwhere(mixed):
        for kind, (dx, dy, dz) in enumerate(KIND_OFFSETS):
            i1, j1, k1 = i + dx, j + dy, k + dz
            if i1 >= G0 or j1 >= G1 or k1 >= G2 or inside[i, j, k] == inside[i1, j1, k1]:
                continue
            lo, hi = ((i1, j1, k1), (i, j, k)) if inside[i, j, k] else ((i, j, k), (i1, j1, k1))
            t = (level - v[lo]) / (v[hi] - v[lo])
            p_lo = np.array([pos[d][lo[d]] for d in range(3)])
            p_hi = np.array([pos[d][hi[d]] for d in range(3)])
            index[(lin(i, j, k), kind)] = len(keys)
            keys.append((lin(i, j, k), kind))
            verts.append(p_lo + t * (p_hi - p_lo))
            ts.append(t)
            ends.append((lo, hi))
            if normals:
                g_lo, g_hi = gradient(v, lo, spacing), gradient(v, hi, spacing)
                g = (1.0 - t) * g_lo + t * g_hi
                n = float(np.sqrt(g @ g))
                gn.append(n)
                gs.append(float(np.linalg.norm(np.abs(g_lo) + np.abs(g_hi))))
                nrm.append(g / n if n > 0 else g)
    # faces: ascending (cube, tetrahedron, triangle)
    faces = []
    cube_mixed = np.zeros((G0 - 1, G1 - 1, G2 - 1), dtype=bool)
    first = inside[:-1, :-1, :-1]
    for code in range(1, 8):
        dx, dy, dz = corner_offset(code)
        cube_mixed |= inside[dx:G0 - 1 + dx, dy:G1 - 1 + dy, dz:G2 - 1 + dz] != first
    for i, j, k in np.argwhere(cube_mixed):
        for q in range(6):
            codes = tet_corner_codes(q)
            corner = [(i + ((c >> 2) & 1), j + ((c >> 1) & 1), k + (c & 1)) for c in codes]
            ins = [bool(inside[c]) for c in corner]
            for tri in tet_triangles(codes, ins):
                f = []
                for a, b in tri:
                    kind = (codes[b] ^ codes[a]) - 1
                    f.append(index[(lin(*corner[a]), kind)])
                faces.append([f[0], f[2], f[1]] if flip else f)
    out = {"verts": np.array(verts, dtype=np.float64).reshape(-1, 3), "faces": np.array(faces, dtype=np.int64).reshape(-1, 3),
           "keys": np.array(keys, dtype=np.int64).reshape(-1, 2), "t": np.array(ts, dtype=np.float64),
           "ends": np.array(ends, dtype=np.int64).reshape(-1, 2, 3)}
    if normals:
        out["normals"] = np.array(nrm, dtype=np.float64).reshape(-1, 3)
        out["gnorm"] = np.array(gn, dtype=np.float64)     # |interpolated gradient|
        out["gscale"] = np.array(gs, dtype=np.float64)    # || |g_lo| + |g_hi| ||: what the interpolation's roundings scale with
    return out


# ---- analytic volumes: v = R - distance to a set, level 0 --------------------------------------------------------------
def lattice_points(shape, aabb):
    p = lattice_positions(shape, aabb)
    return np.stack(np.meshgrid(*p, indexing="ij"), -1)


def sphere_volume(shape, aabb, centre, R):
    return R - np.linalg.norm(lattice_points(shape, aabb) - np.asarray(centre, dtype=np.float64), axis=-1)


def torus_volume(shape, aabb, centre, R, r):
    x = lattice_points(shape, aabb) - np.asarray(centre, dtype=np.float64)
    return r - np.sqrt((np.sqrt(x[..., 0] ** 2 + x[..., 1] ** 2) - R) ** 2 + x[..., 2] ** 2)


def two_spheres_volume(shape, aabb, c0, R0, c1, R1):
    return np.maximum(sphere_volume(shape, aabb, c0, R0), sphere_volume(shape, aabb, c1, R1))


# ---- mesh properties ---------------------------------------------------------------------------------------------------
def directed_edge_counts(faces):
    d = {}
    for a, b, c in np.asarray(faces).tolist():
        for e in ((a, b), (b, c), (c, a)):
            d[e] = d.get(e, 0) + 1
    return d


def edge_use_counts(faces):
    """undirected edge -> number of triangles that use it"""
    u = {}
    for (a, b), n in directed_edge_counts(faces).items():
        e = (min(a, b), max(a, b))
        u[e] = u.get(e, 0) + n
    return u


def is_closed(faces):
    return all(n == 2 for n in edge_use_counts(faces).values())


def boundary_edges(faces):
    return sorted(e for e, n in edge_use_counts(faces).items() if n == 1)


def is_oriented(faces):
    """no edge used more than twice and every directed edge once: an edge two triangles share is used once in each direction"""
    return all(n == 1 for n in directed_edge_counts(faces).values()) and all(n <= 2 for n in edge_use_counts(faces).values())


def euler_characteristic(nv, faces):
    return int(nv) - len(edge_use_counts(faces)) + len(faces)


def signed_volume(verts, faces):
    v = np.asarray(verts, dtype=np.float64)
    f = np.asarray(faces)
    if len(f) == 0:
        return 0.0
    return float(np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)


def all_sign_patterns(rng):
    """256 single-cube volumes: pattern m puts corner code c inside (level 0.5) iff bit c of m is set; random magnitudes"""
    out = []
    for m in range(256):
        v = np.empty((2, 2, 2), dtype=np.float32)
        for c in range(8):
            mag = np.float32(rng.uniform(0.05, 0.45))
            v[tuple(corner_offset(c))] = np.float32(0.5) + (mag if (m >> c) & 1 else -mag)
        out.append(v)
    return out


def tet_edge_set():
    """the 19 edges of the split cube as (corner code of the lower end, kind), per tetrahedron"""
    per = []
    for q in range(6):
        codes = tet_corner_codes(q)
        per.append({(codes[a], (codes[b] ^ codes[a]) - 1) for a, b in itertools.combinations(range(4), 2)})
    return per


# ---- the analytic cases the CPU and the GPU tests share (float32 inputs; the restatement runs once per case) ------------
SHAPE = (24, 24, 24)
AABB = np.array([[-1.0, -1.25, -0.75], [1.0, 1.0, 1.25]], dtype=np.float32)   # a lattice spacing per axis of its own
_cases, _refs = {}, {}


def analytic_cases():
    """name -> (volume float32 [24,24,24], Euler characteristic, analytic enclosed volume); level 0"""
    if not _cases:
        _cases["sphere"] = (sphere_volume(SHAPE, AABB, (0.03, -0.12, 0.21), 0.7).astype(np.float32), 2, 4 / 3 * np.pi * 0.7 ** 3)
        _cases["torus"] = (torus_volume(SHAPE, AABB, (0.02, -0.11, 0.23), 0.55, 0.25).astype(np.float32), 0,
                           2 * np.pi ** 2 * 0.55 * 0.25 ** 2)
        _cases["two_spheres"] = (two_spheres_volume(SHAPE, AABB, (-0.45, -0.1, 0.2), 0.33, (0.5, -0.15, 0.3), 0.3).astype(np.float32),
                                 4, 4 / 3 * np.pi * (0.33 ** 3 + 0.3 ** 3))
    return _cases


def reference(name):
    if name not in _refs:
        _refs[name] = marching_tets(analytic_cases()[name][0], 0.0, AABB, normals=True)
    return _refs[name]


GRADIENT_FLOOR = 2.0 ** -10   # a normal is compared where |interpolated gradient| >= GRADIENT_FLOOR * gscale
