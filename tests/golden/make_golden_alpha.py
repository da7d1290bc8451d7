"""Fixture of the alpha-grid mask (tests/golden/alpha_mask.npz, alpha_mask_ckpt.th), made by the REFERENCE's own
AlphaGridMask.sample_alpha and TensorBase.save (models/tensorBase.py:42-79, :460-470):

    python tests/golden/make_golden_alpha.py        (RODYNRF_REFERENCE=<checkout of the reference>)

A seeded random bool volume of shape (5, 6, 7) with T = 3 -- G2 = 5, G1 = 6, G0 = 7 -- sampled at ~200 points: lattice nodes,
points on cell faces, points just outside the aabb, random interior points; times at the slice centres and at the half-way
values -0.5 / 0.5 (torch.round goes to the even slice).  The checkpoint is a static field on a [9, 11, 7] grid carrying
that mask, written by the reference's save: beside tensors and plain containers it holds the one numpy uint8 array that
save stores under "alphaMask.mask"."""
import contextlib
import io
import os

import numpy as np
import torch

from make_golden import HERE, import_reference

SHAPE, T = (5, 6, 7), 3
AABB = [[-1.5, -1.67, -1.0], [1.5, 1.67, 1.0]]


def main():
    TS = import_reference()[0]
    import models.tensorBase as TB
    g = torch.Generator().manual_seed(11)
    vol = torch.rand(*SHAPE, T, generator=g) < 0.35
    aabb = torch.tensor(AABB)
    mask = TB.AlphaGridMask("cpu", aabb, vol.float(), T)
    G2, G1, G0 = SHAPE
    lin = [torch.linspace(0, 1, n) for n in (G0, G1, G2)]
    node = lambda i, j, k: aabb[0] * (1 - torch.stack([lin[0][i], lin[1][j], lin[2][k]])) + aabb[1] * torch.stack([lin[0][i], lin[1][j], lin[2][k]])
    pts = []
    for _ in range(40):   # lattice nodes
        i, j, k = (int(torch.randint(0, n, (1,), generator=g)) for n in (G0, G1, G2))
        pts.append(node(i, j, k))
    for _ in range(40):   # on a cell face: one coordinate on a node, two inside
        i, j, k = (int(torch.randint(0, n - 1, (1,), generator=g)) for n in (G0, G1, G2))
        p = node(i, j, k) + torch.rand(3, generator=g) * (node(i + 1, j + 1, k + 1) - node(i, j, k))
        ax = int(torch.randint(0, 3, (1,), generator=g))
        p[ax] = node(i, j, k)[ax]
        pts.append(p)
    size = aabb[1] - aabb[0]
    for _ in range(40):   # just outside (within a cell of the box on one axis, some far outside)
        p = aabb[0] + torch.rand(3, generator=g) * size
        ax = int(torch.randint(0, 3, (1,), generator=g))
        off = float(torch.rand(1, generator=g)) * 0.3 * float(size[ax]) / 4 + 1e-4
        p[ax] = aabb[1][ax] + off if torch.rand(1, generator=g) < 0.5 else aabb[0][ax] - off
        pts.append(p)
    pts += [aabb[0].clone(), aabb[1].clone(), aabb[0] - 5.0, aabb[1] + 5.0]
    pts += list(aabb[0] + torch.rand(80, 3, generator=g) * size)
    xyz = torch.stack(pts).float()
    n = xyz.shape[0]
    tvals = torch.tensor([-1.0, 0.0, 1.0, -0.5, 0.5, -0.9, 0.3, 0.74])
    t = tvals[torch.randint(0, tvals.numel(), (n,), generator=g)]
    t[:8] = tvals
    with torch.no_grad():
        ref = mask.sample_alpha(xyz, t)
    out = {"volume": vol.numpy(), "aabb": aabb.numpy(), "xyz": xyz.numpy(), "t": t.numpy(), "alpha": ref.numpy(),
           "gridSize": mask.gridSize.numpy(), "meta.grid": np.array([9, 11, 7])}
    # a static field carrying the mask, written by the reference's own save
    common = dict(density_n_comp=[16, 4, 4], appearance_n_comp=[48, 12, 12], app_dim=27, near_far=[0.0, 1.0],
                  alphaMask_thres=1e-4, density_shift=-10.0, distance_scale=25, pos_pe=6, view_pe=0, featureC=128,
                  step_ratio=2.0, fea2denseAct="relu")
    torch.manual_seed(4)
    with contextlib.redirect_stdout(io.StringIO()):
        st = TS(aabb, [9, 11, 7], T, "cpu", shadingMode="MLP_Fea", fea_pe=2, **common)
    st.alphaMask = mask
    path = os.path.join(HERE, "alpha_mask_ckpt.th")
    st.save(torch.eye(3, 4)[None].repeat(T, 1, 1), torch.tensor(41.5), path)
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    out["ckpt.mask"] = np.asarray(ckpt["alphaMask.mask"])
    out["ckpt.shape"] = np.array(ckpt["alphaMask.shape"])
    np.savez(os.path.join(HERE, "alpha_mask.npz"), **out)
    print("alpha fixture:", n, "points,", int((ref > 0).sum()), "positive,", os.path.getsize(path), "bytes of checkpoint")


if __name__ == "__main__":
    main()
