"""CPU checks of the evaluation path: the eval kernels (camera rays, SSIM) compile for gfx950 with no spill and no scratch,
evaluation_path's time rule, and the new entry points refuse CPU tensors (no fallback)."""
import importlib.util
import os
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("c++filt") is None, reason="needs hipcc")
def test_eval_kernels_do_not_spill():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    rows = {subprocess.run(["c++filt", r["name"]], capture_output=True, text=True).stdout.strip(): r
            for r in kr.table(os.path.join(kr.CSRC, "rdrf_eval.hip"))}
    for w in ("k_camera_rays(", "k_ssim_tile(", "k_ssim_finish("):
        hit = [(n, r) for n, r in rows.items() if w in n]
        assert len(hit) == 1, (w, list(rows))
        name, r = hit[0]
        assert int(r["VGPRs Spill"]) == 0, (name, r["VGPRs Spill"])
        assert int(r["ScratchSize [bytes/lane]"]) == 0, (name, r["ScratchSize [bytes/lane]"])
        assert int(r["Occupancy [waves/SIMD]"]) >= 2, (name, r["Occupancy [waves/SIMD]"])


def test_path_time_follows_evaluation_path():
    import rodynrf
    n = 7
    for idx in range(n):   # renderer.py:1034-1043
        assert rodynrf.path_time("change", idx, n) == round(idx / (n - 1) * (n - 1)) / (n - 1) * 2.0 - 1.0
        assert rodynrf.path_time(0.3, idx, n) == 0.3
    assert rodynrf.path_time("change", 0, 1) == -1.0
    with pytest.raises(ValueError):
        rodynrf.path_time("fixed", 0, 3)


def test_eval_entry_points_refuse_cpu_tensors():
    import rodynrf
    img = torch.rand(16, 16, 3)
    with pytest.raises(rodynrf.RdrfError):
        rodynrf.ssim(img, img)
    with pytest.raises(rodynrf.RdrfError):
        rodynrf.camera_rays(torch.eye(3, 4), 10.0, 4, 5)
    assert rodynrf.RenderMaps._fields == ("rgb", "depth", "acc", "rgb_s", "depth_s", "acc_s", "rgb_d", "depth_d", "acc_d",
                                          "blending")
