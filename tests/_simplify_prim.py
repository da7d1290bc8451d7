"""Vertex clustering restated in plain numpy from the rules of DESIGN.md (section "Mesh simplification") -- not a port of
csrc/rdrf_simplify.hip: int64 keys, a stable argsort, float64 sums through np.add.at (which adds in index order, so a cluster's
members are added in ascending original index), boolean masks for the faces.  The tests decide everything from here.

Conventions (the ones the kernels and the tests must share):
  cell of a vertex   per axis c = clamp(floor(t), 0, n - 1) with t = (v - origin) / cell in fp32 (two roundings); where t >= 0
                     is false (NaN among them) c = 0.  key = (c0 n1 + c1) n2 + c2
  clusters           ascend by key; members ascend by original index
  representative     position float32(float64 sum / count); normal float32(normalised float64 sum), a zero sum stays zero;
                     colour floor((2 sum + k) / (2 k)) per channel
  faces              mapped through the clusters, kept iff the three differ (an index outside [0, V) drops the face); kept
                     faces keep their order and their winding; duplicates stay
  drop_unreferenced  only clusters that a kept face references are emitted, renumbered in ascending key order
  V = 0 or F = 0     nothing is emitted: V' = F' = 0"""
import numpy as np

import _iso_prim as P

CAP_VALUE = -1.0e30


def cells(verts, origin, cell, n):
    """[V,3] int64 cell coordinates"""
    v = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    o, c = np.asarray(origin, dtype=np.float32), np.asarray(cell, dtype=np.float32)
    with np.errstate(all="ignore"):
        t = ((v - o[None]).astype(np.float32) / c[None]).astype(np.float32)
        ok = t >= 0
        f = np.floor(np.where(ok, t, np.float32(0)).astype(np.float64))
    top = np.asarray(n, dtype=np.float64)[None] - 1.0
    return np.where(ok, np.minimum(f, top), 0.0).astype(np.int64)


def keys_of(verts, origin, cell, n):
    c = cells(verts, origin, cell, n)
    return (c[:, 0] * int(n[1]) + c[:, 1]) * int(n[2]) + c[:, 2]


def simplify(verts, faces, origin, cell, n, normals=None, colors=None, drop_unreferenced=True):
    """-> dict(verts f32 [V',3], faces int32 [F',3], remap int32 [V], counts (V', F'), mean f64, abs_sum f64, k int64 [V'],
    normals f32 / nsum f64 / nabs f64, colors u8 where given)"""
    v = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    V, F = len(v), len(f)
    out = {"verts": np.zeros((0, 3), np.float32), "faces": np.zeros((0, 3), np.int32), "remap": np.full(V, -1, np.int32), "counts": (0, 0),
           "mean": np.zeros((0, 3)), "abs_sum": np.zeros((0, 3)), "k": np.zeros(0, np.int64)}
    if normals is not None:
        out.update(normals=np.zeros((0, 3), np.float32), nsum=np.zeros((0, 3)), nabs=np.zeros((0, 3)))
    if colors is not None:
        out["colors"] = np.zeros((0, 3), np.uint8)
    if V == 0 or F == 0:
        return out
    key = keys_of(v, origin, cell, n)
    order = np.argsort(key, kind="stable")
    sk = key[order]
    head = np.ones(V, dtype=bool)
    head[1:] = sk[1:] != sk[:-1]
    cluster = np.empty(V, dtype=np.int64)
    cluster[order] = np.cumsum(head) - 1
    nc = int(head.sum())
    valid = ((f >= 0) & (f < V)).all(1)
    fc = cluster[np.where(valid[:, None], f, 0)]
    keep = valid & (fc[:, 0] != fc[:, 1]) & (fc[:, 1] != fc[:, 2]) & (fc[:, 0] != fc[:, 2])
    used = np.zeros(nc, dtype=bool)
    if drop_unreferenced:
        used[fc[keep].reshape(-1)] = True
    else:
        used[:] = True
    new = np.cumsum(used) - 1
    out["remap"] = np.where(used[cluster], new[cluster], -1).astype(np.int32)
    out["faces"] = new[fc[keep]].astype(np.int32).reshape(-1, 3)
    k = np.bincount(cluster, minlength=nc).astype(np.int64)

    def sums(x):
        s = np.zeros((nc, 3), dtype=np.float64)
        with np.errstate(all="ignore"):
            np.add.at(s, cluster, np.asarray(x, dtype=np.float64))   # sequential, in index order
        return s

    with np.errstate(all="ignore"):
        mean = sums(v) / k[:, None].astype(np.float64)
        out["mean"], out["abs_sum"], out["k"] = mean[used], sums(np.abs(v))[used], k[used]
        out["verts"] = mean[used].astype(np.float32)
        if normals is not None:
            nv = np.asarray(normals, dtype=np.float32).reshape(-1, 3)
            s = sums(nv)
            big = np.abs(s).max(1, keepdims=True)
            scaled = s / np.where(big > 0, big, 1.0)
            length = np.sqrt((scaled * scaled).sum(1, keepdims=True))
            unit = np.where(big > 0, scaled / np.where(big > 0, length, 1.0), s)
            out["normals"], out["nsum"], out["nabs"] = unit[used].astype(np.float32), s[used], sums(np.abs(nv))[used]
    if colors is not None:
        cs = np.zeros((nc, 3), dtype=np.int64)
        np.add.at(cs, cluster, np.asarray(colors, dtype=np.int64).reshape(-1, 3))
        out["colors"] = ((2 * cs + k[:, None]) // (2 * k[:, None]))[used].astype(np.uint8)
    out["counts"] = (int(used.sum()), int(keep.sum()))
    return out


def lattice(aabb, shape, K, cap=False):
    """the lattice of simplify=K over a meshed volume: (origin f32 [3], cell f32 [3], n [3]); cap: the padded volume's"""
    a = np.asarray(aabb, dtype=np.float32).reshape(2, 3)
    G = [int(g) for g in shape[:3]]
    if cap:
        h = (a[1].astype(np.float64) - a[0].astype(np.float64)) / np.array([g - 1 for g in G], dtype=np.float64)
        a = np.stack((a[0].astype(np.float64) - h, a[1].astype(np.float64) + h)).astype(np.float32)
        G = [g + 2 for g in G]
    ext = a[1].astype(np.float64) - a[0].astype(np.float64)
    cell = np.array([K * ext[d] / (G[d] - 1) for d in range(3)], dtype=np.float64).astype(np.float32)
    return a[0].copy(), cell, [-(-(G[d] - 1) // K) for d in range(3)]


def unbalanced_edges(faces):
    """directed edges a -> b whose count differs from that of b -> a (0 on the image of a closed oriented mesh under a
    simplicial map that sends degenerate faces to nothing); self-loops would count too"""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if len(f) == 0:
        return 0
    a = np.concatenate((f[:, 0], f[:, 1], f[:, 2]))
    b = np.concatenate((f[:, 1], f[:, 2], f[:, 0]))
    m = int(max(a.max(), b.max())) + 1
    fwd, n_fwd = np.unique(a * m + b, return_counts=True)
    count = dict(zip(fwd.tolist(), n_fwd.tolist()))
    return sum(1 for e, c in count.items() if count.get((e % m) * m + e // m, 0) != c or e % m == e // m)


_closed = {}


def closed_meshes():
    """name -> (verts f32, faces int64, aabb, shape, cap): the capped ball (a ball larger than its box, closed by cap=True's
    padding), the torus, the sphere and the two spheres of _iso_prim, all closed and oriented"""
    if not _closed:
        for name in ("torus", "sphere", "two_spheres"):
            m = P.reference(name)
            _closed[name] = (m["verts"].astype(np.float32), m["faces"], P.AABB, P.SHAPE, False)
        shape = (12, 12, 12)
        vol = P.sphere_volume(shape, P.AABB, (0.03, -0.12, 0.21), 1.1).astype(np.float32)
        padded = np.full([g + 2 for g in shape], CAP_VALUE, dtype=np.float32)
        padded[1:-1, 1:-1, 1:-1] = vol
        org, cell, _ = lattice(P.AABB, shape, 1, cap=True)
        grown = np.stack((org, (org.astype(np.float64) + cell.astype(np.float64) * (np.array(shape) + 1)).astype(np.float32)))
        m = P.marching_tets(padded, 0.0, grown)
        _closed["capped_ball"] = (m["verts"].astype(np.float32), m["faces"], P.AABB, shape, True)
    return _closed
