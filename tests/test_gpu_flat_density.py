"""The dynamic field's density phase on flat 32-sample tiles (csrc: k_dyn_density_flat + k_ray_scan forward,
k_ray_scan_bwd + k_dyn_density_bwd<., ., true> backward) against the wave-per-ray form it replaced as the training default.
The switch (RDRF_FLAT, read once per process) is live in the tools build only, so each side runs in a child process of
its own on librodynrf_tools.so (built here if missing).  Per shape: the forward outputs must agree BIT FOR BIT (same
arithmetic in the same order), and so must the per-sample input gradient g_xyz under the sorted scatter (a sample's
coordinate gradient is summed in its own lane); under the automatic choice the small batches take the ray-tile scatter,
which sums it over the lanes of the sample's tile slot, so there it agrees to fp32 rounding like the parameter gradients,
g_rays and g_z (tile composition changes the order of the dW partial sums and of d(tout)).  That the deterministic library,
which runs the flat form by default, gives identical parameter gradients run after run is the check of
test_gpu_deterministic.py (complete training steps at S = 40 and at the benchmark's S = 115)."""

import numpy as np
import pytest

from _twin import CHILD, run_twin, tools_lib
from _util import pkg

# S = 115 at the benchmark's 4096 rays (sorted scatter), S = 13 (nvidia_no_poses / davis stage 0), S = 270, and batches
# whose N * S is not a multiple of 32 (the last flat tile is partial)
SHAPES = [(4096, 115), (1024, 13), (1001, 13), (512, 270), (1000, 115)]


def density_case(N, S, mode):
    """what both settings of RDRF_FLAT compute (tests/_det_child.py case)"""
    import torch
    import rodynrf
    N, S = int(N), int(S)
    St = pkg("step")
    RU = pkg("ray_utils")
    L = pkg()
    L.set_scatter_mode(mode)
    torch.manual_seed(0)
    cfg = St.scene_config("nvidia", "stage0")
    dev = torch.device("cuda", 0)
    _, dy = St.build_fields(cfg, dev)
    with torch.no_grad():   # move the time branch and the heads off their initial values a little (reproducibly)
        g = torch.Generator(device=dev).manual_seed(7)
        for p in dy.parameters():
            p.add_(torch.randn(p.shape, device=dev, generator=g) * 0.02 * (p.abs().mean() + 1e-3))
    data = St.SyntheticScene(cfg, dev)
    ids = data.perm[:N]
    rays = RU.generate_rays(ids, data.poses, data.focal, cfg["H"], cfg["W"], ndc=True, near=1.0).detach().clone()
    ts = data.ts_of(ids)
    jit = torch.rand(S, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    xyz, z, valid = rodynrf.sampleXYZ(dy, rays, S, ray_type="ndc", is_train=True, jitter=jit)
    rays.requires_grad_(True)
    xyz = xyz.detach().clone().requires_grad_(True)
    z = z.detach().clone().requires_grad_(True)
    o = dy(rays, ts, None, xyz, z, valid, is_train=True, ray_type="ndc")
    outs = [t for t in o if torch.is_tensor(t) and t.is_floating_point()]
    gen = torch.Generator(device=dev).manual_seed(2)
    loss = sum((t * torch.randn(t.shape, device=dev, generator=gen)).sum() for t in outs if t.requires_grad)
    loss.backward()
    torch.cuda.synchronize()
    res = {f"out{i}": t.detach().cpu().numpy() for i, t in enumerate(outs)}
    res.update(g_xyz=xyz.grad.cpu().numpy(), g_rays=rays.grad.cpu().numpy(),
               g_z=(z.grad if z.grad is not None else torch.zeros(1)).cpu().numpy())
    for n, p in dy.named_parameters():
        if p.grad is not None:
            res["p." + n] = p.grad.cpu().numpy()
    return res


def _run(tmp_path, N, S, flat, mode):
    res = run_twin(tmp_path, [CHILD, "case", "test_gpu_flat_density", "density_case", str(N), str(S), mode], lib=tools_lib(),
                   extra_env={"RDRF_FLAT": flat})
    return {k: v.numpy() for k, v in res.items()}


def _rel(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["auto", "sorted"])
@pytest.mark.parametrize("N,S", SHAPES)
def test_flat_density_phase_matches_wave_per_ray(tmp_path, N, S, mode):
    base = _run(tmp_path, N, S, "0", mode)
    flat = _run(tmp_path, N, S, "1", mode)
    assert sorted(base) == sorted(flat)
    bad = []
    for k in sorted(base):
        a, b = flat[k], base[k]
        if k.startswith("out") or (k == "g_xyz" and mode == "sorted"):
            if a.shape != b.shape or not np.array_equal(a.view(np.uint32), b.view(np.uint32)):
                nd = int((a != b).sum()) if a.shape == b.shape else -1
                bad.append(f"{k}: {nd} entries differ in their bits (max |diff| "
                           f"{float(np.abs(a - b).max()) if nd >= 0 else float('nan'):.3e})")
        else:
            r = _rel(a, b)
            if not r <= 2e-5:
                bad.append(f"{k}: rel. L2 {r:.3e}")
    assert not bad, "\n".join(bad)

