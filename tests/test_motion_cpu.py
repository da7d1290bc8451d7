"""CPU checks of the evaluation render's motion maps: the new kernels' register budget (hipcc cross-compiles gfx950
without a GPU), the package surface, the two C structs' sizes against the header's field lists, and the reference fixtures
tests/golden/motion_{ndc,contract}.npz against the conditions their generator (make_golden_motion.py) asserts."""
import ctypes as C
import importlib
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from _util import pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOTION = ("flow_f", "flow_b", "flow_s_f", "flow_s_b", "delta_xyz")


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("c++filt") is None, reason="needs hipcc")
def test_motion_kernels_do_not_spill():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    rows = {subprocess.run(["c++filt", r["name"]], capture_output=True, text=True).stdout.strip(): r
            for r in kr.table(os.path.join(kr.CSRC, "rdrf_motion.hip"))}
    for w in ("k_motion_maps<true>(", "k_motion_maps<false>(", "k_flow_radmax(", "k_flow_colors("):
        hit = [(n, r) for n, r in rows.items() if w in n]
        assert len(hit) == 1, (w, list(rows))
        name, r = hit[0]
        assert int(r["VGPRs"]) <= 256, (name, r["VGPRs"])
        assert int(r["VGPRs Spill"]) == 0, (name, r["VGPRs Spill"])
        assert int(r["ScratchSize [bytes/lane]"]) == 0, (name, r["ScratchSize [bytes/lane]"])
        assert int(r["Occupancy [waves/SIMD]"]) >= 2, (name, r["Occupancy [waves/SIMD]"])


def test_motion_surface_is_exported():
    import rodynrf
    L = pkg()
    assert rodynrf.MotionMaps._fields == MOTION
    for name in ("MotionMaps", "flow_to_image", "delta_xyz_image", "render_rays", "render_frame", "render_view"):
        assert name in rodynrf.__all__ and hasattr(rodynrf, name), name
    for sym in ("rdrf_render_motion_fwd", "rdrf_render_motion_workspace_bytes", "rdrf_flow_to_image",
                "rdrf_flow_to_image_workspace_bytes"):
        assert sym in L.SYMBOLS and hasattr(L.lib, sym), sym
    for N, S in ((1, 13), (512, 115), (32400, 115)):
        assert L.lib.rdrf_render_motion_workspace_bytes(N, S) >= L.lib.rdrf_render_workspace_bytes(N, S)
    # no CPU fallback
    with pytest.raises(rodynrf.RdrfError):
        rodynrf.flow_to_image(torch.zeros(4, 4, 2))
    d = torch.tensor([[[0.5, -1.0, 0.25]]])
    assert torch.equal(rodynrf.delta_xyz_image(d), (d / 1.0 + 1.0) / 2.0)


def _header_struct(name):
    hdr = open(os.path.join(ROOT, "include", "rodynrf.h")).read()
    body = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + ";", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        typ = "ptr" if "*" in decl else ("i64" if "int64_t" in decl else "int")
        for nm in decl.replace("*", " ").split(",") if typ != "ptr" else [decl]:
            fields.append((nm.split()[-1].strip("* "), typ))
    return fields


def test_struct_sizes_match_the_header():
    L = pkg()
    ctype = {"ptr": C.c_void_p, "int": C.c_int, "i64": C.c_int64}
    for name, cls in (("RdrfMotionMaps", L.MotionMapsC), ("RdrfMotionCams", L.MotionCamsC)):
        fields = _header_struct(name)
        assert [f for f, _ in fields] == [f for f, _ in cls._fields_], (name, fields)

        class Mirror(C.Structure):
            _fields_ = [(f, ctype[t]) for f, t in fields]
        assert C.sizeof(cls) == C.sizeof(Mirror), name
        for f, _ in fields:
            assert getattr(cls, f).offset == getattr(Mirror, f).offset, (name, f)
    assert C.sizeof(L.MotionMapsC) == 40 and C.sizeof(L.MotionCamsC) == 40
    assert tuple(f for f, _ in L.MotionMapsC._fields_) == MOTION == L.MOTION_MAPS


@pytest.mark.parametrize("case", ["motion_ndc", "motion_contract"])
def test_motion_fixture_is_worth_having(case):
    from _util import GOLDEN
    path = os.path.join(GOLDEN, case + ".npz")
    assert os.path.getsize(path) < 1 << 20
    z = np.load(path)
    H, W, S = int(z["meta.H"]), int(z["meta.W"]), int(z["meta.S"])
    assert (W, H) == (24, 16) and z["rays"].shape == (H * W, 6) and z["ts"].shape == (H * W,)
    for k in MOTION:
        assert z["out." + k].shape == (H * W, 3 if k == "delta_xyz" else 2) and np.isfinite(z["out." + k]).all(), k
    # the generator's asserts, on the stored file
    assert np.median(np.abs(z["out.flow_f"] - z["out.flow_s_f"])) >= 1.0
    assert np.median(np.abs(z["out.flow_b"] - z["out.flow_s_b"])) >= 1.0
    assert np.abs(z["out.delta_xyz"]).max() > 1e-3
    assert (z["out.acc_d"] > 0.1).mean() >= 0.5
    assert float(z["stat.fp64_spread"]) <= 2e-5
    for k in MOTION[:4]:
        assert z["viz." + k].shape == (H, W, 3) and z["viz." + k].dtype == np.uint8
    assert (z["viz_nan.image"] == 255).all() and (z["viz_zero.image"] == 255).all()
    assert np.isinf(z["viz_inf.flow"]).sum() == 2 and np.isnan(z["viz_nan.flow"]).sum() == 1
