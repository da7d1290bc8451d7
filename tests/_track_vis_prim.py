"""Float64 reference of the per-slot visibility of a point track (rdrf_track_visibility_fwd, include/rodynrf.h), shared by
test_track_vis_cpu.py and test_gpu_track_vis.py.  No GPU.

    F_s(d) = (1 - (1 - exp(-sigma_d d)) b) (1 - (1 - exp(-sigma_s d)) (1 - b)) + 1e-10        (raw2outputs' T_full factor)
    vis    = prod_{s < j} F_s(dists_s) * F_j(dq),   j = the last sample with z_j <= zq,
    dq     = dists_j * min(zq - z_j, z_{j+1} - z_j) / (z_{j+1} - z_j)   (0 for the last sample: its interval has no width)

zq < z_0 gives exactly 1.  The arrays are fp32 numbers widened to float64, so both sides see the same values."""
import numpy as np
import torch


def factor(sigma_s, sigma_d, blending, d):
    a_d = 1.0 - torch.exp(-sigma_d * d)
    a_s = 1.0 - torch.exp(-sigma_s * d)
    return (1.0 - a_d * blending) * (1.0 - a_s * (1.0 - blending)) + 1e-10


def visibility(z, dists, sigma_s, sigma_d, blending, zq):
    """z, dists, sigma_s, sigma_d, blending [N,S], zq [N] -> (vis [N], j [N]) in float64; j = -1 where zq < z_0"""
    z, dists, sigma_s, sigma_d, blending = (torch.as_tensor(np.asarray(t)).double() for t in (z, dists, sigma_s, sigma_d, blending))
    zq = torch.as_tensor(np.asarray(zq)).double()
    N, S = z.shape
    j = (z <= zq[:, None]).sum(-1) - 1
    s = torch.arange(S)[None]
    width = torch.cat([z[:, 1:] - z[:, :-1], torch.zeros(N, 1, dtype=torch.float64)], -1)
    frac = torch.where(width > 0, ((zq[:, None] - z).clamp(min=0.0) / width.clamp(min=1e-300)).clamp(max=1.0), torch.zeros_like(z))
    d = torch.where(s == j[:, None], frac * dists, dists)
    f = factor(sigma_s, sigma_d, blending, d)
    f = torch.where(s <= j[:, None], f, torch.ones_like(f))
    return f.prod(-1), j


def t_full(dists, sigma_s, sigma_d, blending):
    """raw2outputs' T_full [N,S] from its own formula (renderer.py:236-245), float64"""
    dists, sigma_s, sigma_d, blending = (torch.as_tensor(np.asarray(t)).double() for t in (dists, sigma_s, sigma_d, blending))
    f = factor(sigma_s, sigma_d, blending, dists)
    one = torch.ones_like(f[:, :1])
    return torch.cumprod(torch.cat([one, f], -1), -1)[:, :-1]


# ---- the slot's ray and depth (step 1 and 2 of the contract), float64 ---------------------------------------------------
def slot_geometry(O, p, c2w, focal, H, W, ray_type):
    """p [N,3] field coordinates, c2w [N,3,4] -> (pix [N,2], cam [N,3], zstar [N]) by the oracle's own functions"""
    world = O.ndc2world(p, H, W, focal) if ray_type == "ndc" else O.contract2world(p)
    pix, _ = O._project(world, H, W, focal, c2w)
    q = world - c2w[..., 3]
    cam = (q[..., None, :] * c2w[..., :3, :3].transpose(-1, -2)).sum(-1)
    if ray_type == "ndc":
        zstar = (torch.clamp(p[..., 2], min=-1.0, max=1.0 - 1e-6) + 1.0) / 2.0
    else:
        zstar = -cam[..., 2]
    return pix, cam, zstar


def poses9_of(c2w):
    """the 9-vector poses whose pose_to_mtx is c2w (orthonormal c2w: Gram-Schmidt changes nothing beyond rounding)"""
    return torch.cat([c2w[..., :, 0], c2w[..., :, 1], c2w[..., :, 3]], -1)


def zq_rounding(cam_terms, zstar, zq, ray_type):
    """bound of |fp32 zq - exact zq| for the kernel's arithmetic, in absolute terms.
    ndc: z* = (c + 1) / 2 is one rounded sum (the halving is exact), zq = z* - margin one more: 2^-24 (|z*| + |zq|).
    contract: z* = -cam_z = -sum_j (world_j - c_j) R_j2: world_j carries four roundings (n - 2, -1 / ., p / n, the product),
    the difference one, each product one, the two sums one each: at most 8 half-ulps of (|world_j| + |c_j|) |R_j2| summed over
    j (`cam_terms`), plus the rounding of z* - margin."""
    u = 2.0 ** -24
    if ray_type == "ndc":
        return u * (zstar.abs() + zq.abs())
    return u * (8.0 * cam_terms + zq.abs())
