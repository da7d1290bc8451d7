"""CPU checks of the alpha-mask layer: the restatement of tests/_alpha_prim.py is pinned against the reference-made fixture
(tests/golden/alpha_mask.npz, make_golden_alpha.py) and against F.max_pool3d / F.grid_sample / np.packbits; the kernels of
csrc/rdrf_alpha.hip compile for gfx950 without spills or scratch at two waves per SIMD; the ISA lint of the bf16 MFMAs
finds nothing in the unit."""
import importlib.util
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _alpha_prim as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _fixture():
    z = np.load(os.path.join(GOLDEN, "alpha_mask.npz"))
    return {k: z[k] for k in z.files}


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_sample_alpha_restatement_matches_the_reference_fixture():
    g = _fixture()
    got = A.sample_alpha(g["volume"], g["aabb"], g["xyz"], g["t"])
    assert np.abs(got - g["alpha"]).max() <= 1e-6
    assert np.array_equal(got > 0, g["alpha"] > 0)
    assert (g["alpha"] > 0).sum() > 50 and (g["alpha"] == 0).sum() > 20
    # half-way times go to the even slice
    assert A.time_slice([-0.5, 0.5, -1.0, 0.0, 1.0], 3).tolist() == [0, 2, 0, 1, 2]
    assert list(g["gridSize"]) == [7, 6, 5]


def test_sample_alpha_restatement_matches_grid_sample():
    rng = np.random.default_rng(3)
    occ = rng.random((4, 9, 5, 2)) < 0.4
    aabb = np.array([[-1.0, -2.0, 0.5], [2.0, 1.0, 1.5]], dtype=np.float32)
    xyz = (aabb[0] + rng.random((300, 3)) * (aabb[1] - aabb[0]) * 1.2 - 0.1).astype(np.float32)
    for k, t in enumerate((-1.0, 1.0)):
        vol = torch.from_numpy(occ[..., k].astype(np.float32))[None, None]
        gn = (torch.from_numpy(xyz) - torch.from_numpy(aabb[0])) * (1.0 / torch.from_numpy(aabb[1] - aabb[0]) * 2) - 1
        ref = F.grid_sample(vol, gn.view(1, -1, 1, 1, 3), align_corners=True).view(-1).numpy()
        got = A.sample_alpha(occ, aabb, xyz, t)
        assert np.abs(got - ref).max() <= 1e-6
        assert np.array_equal(got > 0, ref > 0)


@pytest.mark.parametrize("shape", [(3, 4, 5, 2), (1, 1, 1, 3), (9, 11, 7, 3)])
def test_pool_threshold_pack_restatement(shape):
    rng = np.random.default_rng(sum(shape))
    thres = 0.3
    alpha = (rng.random(shape) * 1.4 - 0.2).astype(np.float32)
    alpha.reshape(-1)[:: 7] = np.float32(thres)   # values exactly at the threshold are occupied
    a = torch.from_numpy(alpha).clamp(0, 1).transpose(0, 2).contiguous()[None]          # models/tensorBase.py:595-603
    p = F.max_pool3d(torch.permute(a, (0, 4, 1, 2, 3)), kernel_size=3, padding=1, stride=1)
    ref = (torch.permute(p[0], (1, 2, 3, 0)) >= thres).numpy()
    occ = A.pool_threshold(alpha, thres)
    assert np.array_equal(occ, ref)
    assert np.array_equal(A.pack(occ), np.packbits(ref.reshape(-1)))
    st = A.stats(occ)
    assert st[0] == int(ref.sum())
    if st[0]:
        iz, iy, ix, _ = np.nonzero(ref)
        assert st[1:] == [ix.min(), iy.min(), iz.min(), ix.max(), iy.max(), iz.max()]


def test_single_corner_voxel_does_not_wrap():
    alpha = np.zeros((4, 5, 6, 2), dtype=np.float32)
    alpha[3, 4, 5, 1] = 1.0
    occ = A.pool_threshold(alpha, 0.5)
    assert occ.sum() == 8 and occ[4:, 3:, 2:, 1].all() and not occ[..., 0].any()
    assert A.stats(occ) == [8, 2, 3, 4, 3, 4, 5]
    assert A.stats(A.pool_threshold(np.zeros((2, 2, 2, 2)), 0.5)) == [0]


def test_fixture_checkpoint_payload_is_the_packed_volume():
    g = _fixture()
    assert np.array_equal(g["ckpt.mask"], A.pack(g["volume"]))
    assert list(g["ckpt.shape"]) == [1, 1, 5, 6, 7, 3]
    ckpt = torch.load(os.path.join(GOLDEN, "alpha_mask_ckpt.th"), map_location="cpu", weights_only=False)
    assert np.array_equal(np.asarray(ckpt["alphaMask.mask"]), g["ckpt.mask"])
    assert torch.equal(ckpt["alphaMask.aabb"], torch.from_numpy(g["aabb"]))


def test_package_exposes_the_alpha_surface_and_refuses_cpu_tensors():
    import rodynrf
    L = rodynrf._lib
    for sym in ("rdrf_compute_alpha_workspace_bytes", "rdrf_compute_alpha", "rdrf_alpha_mask_build", "rdrf_alpha_mask_sample",
                "rdrf_alpha_mask_valid"):
        assert sym in L.SYMBOLS and hasattr(L.lib, sym), sym
    for name in ("compute_alpha", "getDenseAlpha", "updateAlphaMask", "filtering_rays"):
        assert callable(getattr(rodynrf.TensorBase, name))
    g = _fixture()
    m = rodynrf.AlphaGridMask("cpu", torch.from_numpy(g["aabb"]), torch.from_numpy(g["volume"]).float(), 3)
    assert m.gridSize.tolist() == [7, 6, 5] and m.tSize == 3 and m.shape == (1, 1, 5, 6, 7, 3)
    assert np.array_equal(m.packed.numpy(), g["ckpt.mask"])                      # packed as np.packbits would
    assert torch.equal(m.alpha_volume[0, 0].bool(), torch.from_numpy(g["volume"]))
    with pytest.raises(rodynrf.RdrfError):   # no CPU fallback
        m.sample_alpha(torch.zeros(4, 3), 0.0)
    assert L.lib.rdrf_compute_alpha_workspace_bytes(1000, 12) >= 12 * 32 * 4


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("c++filt") is None, reason="needs hipcc")
def test_alpha_kernels_do_not_spill():
    kr = _tool("kernel_resources")
    rows = {subprocess.run(["c++filt", r["name"]], capture_output=True, text=True).stdout.strip(): r
            for r in kr.table(os.path.join(kr.CSRC, "rdrf_alpha.hip"))}
    for w in ("k_alpha_dyn(", "k_alpha_static(", "k_alpha_time_branch(", "k_alpha_mask_build(", "k_alpha_mask_sample("):
        hit = [(n, r) for n, r in rows.items() if w in n]
        assert len(hit) == 1, (w, list(rows))
        name, r = hit[0]
        assert int(r["VGPRs Spill"]) == 0, (name, r["VGPRs Spill"])
        assert int(r["ScratchSize [bytes/lane]"]) == 0, (name, r["ScratchSize [bytes/lane]"])
        assert int(r["Occupancy [waves/SIMD]"]) >= 2, (name, r["Occupancy [waves/SIMD]"])


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_alpha_unit_passes_the_mfma_hazard_lint():
    mh = _tool("mfma_hazards")
    src = os.path.join(ROOT, "robust-dynrf_amd", "csrc", "rdrf_alpha.hip")
    assert "rdrf_alpha.hip" not in [os.path.basename(u) for u in mh.UNITS]   # the product set of the lint stays as it is
    results = mh.run([src])
    kernels = [(k, r) for _, k, r in results if k]
    assert [k for k, _ in kernels if "k_alpha_dyn" in k], results   # the density head's first layer is bf16 x 3
    floor_raw = min(v[2] for v in mh.read_table(os.path.join(ROOT, "profiles", "r09_mfma_hazards_parent.txt")).values())
    for k, r in kernels:   # the findings of tests/test_mfma_hazards_cpu.py, none allowed
        assert r["n"] >= 108, (k, r["n"])   # head_layer1: nine K = 16 steps x 2 output blocks x the six products of bf16 x 3
        assert len(r["unchecked"]) <= 0.05 * r["n"], (k, r["unchecked"])
        assert min(r["war"], default=mh.NONE) > 2, (k, min(r["war"]))
        assert min(r["raw"], default=mh.NONE) >= floor_raw, (k, min(r["raw"]), floor_raw)
