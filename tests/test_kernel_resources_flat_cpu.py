"""Register budget of the flat-tile density phase (the dynamic field's training default): the training instantiation of
k_dyn_density_flat, the scan kernels on either side of it (k_ray_scan, k_ray_scan_bwd) and the flat k_dyn_density_bwd<0/1>
compile to at most 256 registers with no spill and no scratch (hipcc cross-compiles gfx950 without a GPU)."""
import importlib.util
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _table(kr, src):
    out = {}
    for r in kr.table(os.path.join(kr.CSRC, src)):
        out[subprocess.run(["c++filt", r["name"]], capture_output=True, text=True).stdout.strip()] = r
    return out


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("c++filt") is None, reason="needs hipcc")
def test_flat_density_phase_kernels_do_not_spill():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    rows = {**_table(kr, "rdrf_fwd.hip"), **_table(kr, "rdrf_bwd.hip")}
    want = ["k_dyn_density_flat<true>(", "k_dyn_density_flat<false>(", "k_ray_scan(", "k_ray_scan_bwd(",
            "k_dyn_density_bwd<0, false, true>(", "k_dyn_density_bwd<1, false, true>("]
    for w in want:
        hit = [(n, r) for n, r in rows.items() if w in n]
        assert len(hit) == 1, (w, [n for n, _ in hit])
        name, r = hit[0]
        assert int(r["VGPRs"]) <= 256, (name, r["VGPRs"])
        assert int(r["VGPRs Spill"]) == 0, (name, r["VGPRs Spill"])
        assert int(r["ScratchSize [bytes/lane]"]) == 0, (name, r["ScratchSize [bytes/lane]"])
        assert int(r["Occupancy [waves/SIMD]"]) >= 2, (name, r["Occupancy [waves/SIMD]"])
