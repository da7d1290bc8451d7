"""numpy / torch restatement of the alpha-mask primitives (csrc/rdrf_alpha.hip): pool, threshold, pack, box and
sample_alpha, written from the reference's models/tensorBase.py:42-79, :465-469, :592-629 and pinned against
F.max_pool3d / F.grid_sample / np.packbits and the reference-made fixture by tests/test_alpha_cpu.py."""
import numpy as np
import torch


def pool_threshold(alpha, thres):
    """alpha [G0,G1,G2,T] -> bool occupancy [G2,G1,G0,T]: clamp, 3x3x3 max over space per time slice (edges see fewer
    cells: padding never wins), >= thres.  Plain shifted maxima -- no F.max_pool3d here."""
    a = np.clip(np.asarray(alpha, dtype=np.float32), 0.0, 1.0).transpose(2, 1, 0, 3)
    out = a.copy()
    for ax in range(3):
        src = out.copy()
        lo = [slice(None)] * 4
        hi = [slice(None)] * 4
        lo[ax], hi[ax] = slice(1, None), slice(None, -1)
        out[tuple(lo)] = np.maximum(out[tuple(lo)], src[tuple(hi)])
        out[tuple(hi)] = np.maximum(out[tuple(hi)], src[tuple(lo)])
    return out >= np.float32(thres)


def pack(occ):
    """bool [G2,G1,G0,T] -> the checkpoint payload: C-order flattening, eight entries per byte, first in the top bit"""
    flat = np.asarray(occ, dtype=bool).reshape(-1)
    flat = np.concatenate([flat, np.zeros((-flat.size) % 8, dtype=bool)]).reshape(-1, 8)
    return (flat * np.array([128, 64, 32, 16, 8, 4, 2, 1])).sum(1).astype(np.uint8)


def stats(occ):
    """-> [count, min ix, iy, iz, max ix, iy, iz] over all times (the six indices are undefined for count 0)"""
    occ = np.asarray(occ, dtype=bool)
    iz, iy, ix, _ = np.nonzero(occ)
    if ix.size == 0:
        return [0]
    return [int(ix.size), int(ix.min()), int(iy.min()), int(iz.min()), int(ix.max()), int(iy.max()), int(iz.max())]


def time_slice(t, T):
    """round((t + 1) / 2 (T - 1)) in float32, half-way cases to even"""
    t = np.asarray(t, dtype=np.float32)
    return np.rint((t + np.float32(1)) / np.float32(2) * np.float32(T - 1)).astype(np.int64)


def sample_alpha(occ, aabb, xyz, t):
    """occ bool [G2,G1,G0,T], aabb [2,3], xyz [n,3], t scalar or [n] -> float32 [n]: trilinear, align_corners, zero padding"""
    f32 = np.float32
    occ = np.asarray(occ, dtype=bool)
    G2, G1, G0, T = occ.shape
    aabb = np.asarray(aabb, dtype=f32)
    xyz = np.asarray(xyz, dtype=f32).reshape(-1, 3)
    inv = f32(1.0) / (aabb[1] - aabb[0]) * f32(2)
    g = (xyz - aabb[0]) * inv - f32(1)
    k = np.broadcast_to(time_slice(t, T), (xyz.shape[0],))
    f = [((g[:, d] + f32(1)) / f32(2)) * f32(n - 1) for d, n in enumerate((G0, G1, G2))]
    with np.errstate(invalid="ignore"):
        f0 = [np.floor(v) for v in f]
    out = np.zeros(xyz.shape[0], dtype=f32)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                w = np.ones(xyz.shape[0], dtype=f32)
                idx = []
                ok = np.ones(xyz.shape[0], dtype=bool)
                for d, (o, n) in enumerate(zip((dx, dy, dz), (G0, G1, G2))):
                    w = w * ((f[d] - f0[d]) if o else ((f0[d] + f32(1)) - f[d]))
                    c = f0[d] + o
                    ok &= (c >= 0) & (c <= n - 1)
                    idx.append(np.where(ok, c, 0).astype(np.int64))
                v = occ[idx[2], idx[1], idx[0], k] & ok
                out = out + np.where(v, w, f32(0)).astype(f32)
    return out


def bbox_filter(aabb, rays):
    """the bbox_only branch of filtering_rays (models/tensorBase.py:646-656)"""
    aabb, rays = torch.as_tensor(aabb), torch.as_tensor(rays)
    o, d = rays[..., :3], rays[..., 3:6]
    vec = torch.where(d == 0, torch.full_like(d, 1e-6), d)
    ra, rb = (aabb[1] - o) / vec, (aabb[0] - o) / vec
    return torch.maximum(ra, rb).amin(-1) > torch.minimum(ra, rb).amax(-1)
