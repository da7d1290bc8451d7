"""CPU-side checks of the world-space ray path: the new C symbols are declared and exported (ABI version unchanged), and
the fixture tests/golden/world.npz is what its generator promises -- its sample_ray vectors follow from its rays by a
plain fp32 torch restatement, bit for bit, and its ray set has the required mix."""
import os
import re

import numpy as np
import torch

from _util import GOLDEN, pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rdrf_sample_world", "rdrf_sample_world_bwd", "rdrf_render_world_fwd")


def test_header_declares_and_library_exports_the_world_symbols():
    L = pkg()
    hdr = open(os.path.join(ROOT, "include", "rodynrf.h")).read()
    declared = set(re.findall(r"\b(rdrf_[a-z0-9_]+)\s*\(", hdr))
    for sym in NEW_SYMBOLS:
        assert sym in declared, f"include/rodynrf.h does not declare {sym}"
        assert hasattr(L.lib, sym), f"librodynrf.so does not export {sym}"
        assert sym in L.SYMBOLS
    # purely additive: no struct or existing signature changed
    assert L.lib.rdrf_abi_version() == L.ABI_VERSION == 6
    assert int(re.search(r"#define RDRF_ABI_VERSION (\d+)", hdr).group(1)) == 6
    assert "RDRF_RAY_OTHER = 2" in hdr and L.RAY_TYPES == {"ndc": 0, "contract": 1}


def test_fields_have_sample_ray_and_the_reference_step():
    import rodynrf
    g = np.load(os.path.join(GOLDEN, "world.npz"))
    kw = dict(density_n_comp=[16, 4, 4], appearance_n_comp=[48, 12, 12], app_dim=27, near_far=[0.5, 4.0], alphaMask_thres=1e-4,
              density_shift=-1.0, distance_scale=25, pos_pe=6, view_pe=0, featureC=128, step_ratio=float(g["meta.step_ratio"]))
    aabb, grid = torch.from_numpy(g["aabb"]), [int(v) for v in g["meta.grid"]]
    st = rodynrf.TensorVMSplit(aabb, grid, 12, "cpu", shadingMode="MLP_Fea", fea_pe=2, **kw)
    dy = rodynrf.TensorVMSplit_TimeEmbedding(aabb, grid, 12, "cpu", shadingMode="MLP_Fea_late_view", fea_pe=0, **kw)
    for f in (st, dy):
        assert callable(getattr(f, "sample_ray"))
        assert np.float32(f._step_host) == g["meta.stepSize"] == f.stepSize.numpy()


def _sample_ray_fp32(rays, aabb, near, far, step, S, u=None):
    """the world-space march in fp32 torch operations, one rounding each"""
    o, d = rays[:, :3], rays[:, 3:]
    vec = torch.where(d == 0, torch.full_like(d, 1e-6), d)
    t_min = torch.minimum((aabb[1] - o) / vec, (aabb[0] - o) / vec).amax(-1).clamp(min=near, max=far)
    rng = torch.arange(S)[None].float()
    if u is not None:
        rng = rng.repeat(rays.shape[0], 1) + u[:, None]
    z = t_min[:, None] + step * rng
    xyz = o[:, None, :] + d[:, None, :] * z[..., None]
    return xyz, z, ~((aabb[0] > xyz) | (xyz > aabb[1])).any(-1)


def test_fixture_sampler_restated_bit_for_bit():
    g = np.load(os.path.join(GOLDEN, "world.npz"))
    rays, aabb = torch.from_numpy(g["rays"]), torch.from_numpy(g["aabb"])
    near, far = (float(v) for v in g["meta.near_far"])
    step, u = torch.from_numpy(g["meta.stepSize"]), torch.from_numpy(g["u"])
    assert rays.shape == (67, 6) and u.shape == (67,)
    for S in (33, 70):
        for mode in ("eval", "train"):
            xyz, z, valid = _sample_ray_fp32(rays, aabb, near, far, step, S, u if mode == "train" else None)
            pre = f"{mode}{S}."
            assert np.array_equal(z.numpy(), g[pre + "z"]), pre
            assert np.array_equal(xyz.numpy(), g[pre + "xyz"]), pre
            assert np.array_equal(valid.numpy(), g[pre + "valid"]), pre


def test_fixture_ray_mix():
    """25-75 % of all samples valid (and of each sampler call); rays through all six faces with the clamp inactive, rays
    clamped to near (origin inside) and to far, at least three complete misses, trailing invalid runs, exact-zero direction
    components; no tie between two axes and no t_min within 1e-3 of near / far unless clamped"""
    g = np.load(os.path.join(GOLDEN, "world.npz"))
    kind = g["kind"]
    fracs = [g[f"{m}{S}.valid"].mean() for S in (33, 70) for m in ("eval", "train")]
    assert all(0.25 <= f <= 0.75 for f in fracs), fracs
    allv = np.concatenate([g[f"{m}{S}.valid"].reshape(-1) for S in (33, 70) for m in ("eval", "train")]).mean()
    assert 0.25 <= allv <= 0.75
    r = torch.from_numpy(g["rays"]).double()
    lo, hi = (torch.from_numpy(g["aabb"][i]).double() for i in (0, 1))
    near, far = (float(v) for v in g["meta.near_far"])
    vec = torch.where(r[:, 3:] == 0, torch.full_like(r[:, 3:], 1e-6), r[:, 3:])
    ra, rb = (hi - r[:, :3]) / vec, (lo - r[:, :3]) / vec
    m = torch.minimum(ra, rb)
    top = m.sort(-1, descending=True)[0]
    assert float((top[:, 0] - top[:, 1]).min()) > 1e-3
    raw, axis = m.max(-1)
    assert float((raw - near).abs().min()) > 1e-3 and float((raw - far).abs().min()) > 1e-3
    free = (raw > near) & (raw < far)
    upper = (ra < rb).gather(1, axis[:, None])[:, 0]
    faces = {(int(a), bool(u_)) for a, u_, f in zip(axis, upper, free) if f}
    assert len(faces) == 6
    assert int((raw < near).sum()) >= 3 and int((raw > far).sum()) >= 3
    for S in (33, 70):
        v = g[f"eval{S}.valid"]
        assert int((~v.any(1)).sum()) >= 3 and not v[kind == 8].any()
        assert int((v[:, 0] & ~v[:, -1]).sum()) >= 6                       # leaves the box before the last sample
        inside = raw < near
        assert v[inside.numpy(), 0].all()                                   # starts inside: valid from the first sample
    assert int(((r[:, 3:] == 0).sum(-1) == 1).sum()) >= 3
