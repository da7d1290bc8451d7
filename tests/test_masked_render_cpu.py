"""The masked render without a GPU: its C ABI is declared, bound and exported by both libraries, the ABI version stands, its
workspace holds the unmasked render's and grows with N and S, and its kernels fit their registers without scratch."""
import ctypes as C
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "robust-dynrf_amd")
NEW = ("rdrf_render_masked_ws_bytes", "rdrf_render_masked_fwd")


def _lib_source():
    return open(os.path.join(PKG, "_lib.py")).read()


def test_entry_points_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "rodynrf.h")).read()
    declared = set(re.findall(r"\b(rdrf_[a-z0-9_]+)\s*\(", hdr))
    src = _lib_source()
    table = re.search(r"^SIGNATURES = \{\n(.*?)^\}", src, re.S | re.M).group(1)   # name -> (restype, argtypes); _load applies it
    assert re.search(r"^SYMBOLS = list\(SIGNATURES\)$", src, re.M), "_lib.SYMBOLS is not the signature table's key list"
    for sym in NEW:
        assert sym in declared, f"{sym} is not declared in include/rodynrf.h"
        assert re.search(rf'^    "{sym}": \(\w+, \[\w', table, re.M), f"{sym} has no ctypes signature (and so is not in _lib.SYMBOLS)"
    for so in ("librodynrf.so", "librodynrf_det.so"):
        lib = C.CDLL(os.path.join(PKG, so))
        for sym in NEW:
            assert hasattr(lib, sym), f"{so} does not export {sym}"


def test_abi_version_is_still_6():
    hdr = open(os.path.join(ROOT, "include", "rodynrf.h")).read()
    assert re.search(r"#define RDRF_ABI_VERSION (\d+)", hdr).group(1) == "6"
    assert re.search(r"^ABI_VERSION = (\d+)", _lib_source(), re.M).group(1) == "6"
    lib = C.CDLL(os.path.join(PKG, "librodynrf.so"))
    assert lib.rdrf_abi_version() == 6


def test_workspace_holds_the_unmasked_render_and_is_monotone():
    lib = C.CDLL(os.path.join(PKG, "librodynrf.so"))
    for f in (lib.rdrf_render_masked_ws_bytes, lib.rdrf_render_workspace_bytes):
        f.restype, f.argtypes = C.c_size_t, [C.c_int, C.c_int]
    Ns, Ss = (1, 7, 64, 257, 512, 32400), (1, 13, 31, 33, 115, 270)
    size = {(n, s): lib.rdrf_render_masked_ws_bytes(n, s) for n in Ns for s in Ss}
    for (n, s), b in size.items():
        assert b >= lib.rdrf_render_workspace_bytes(n, s), (n, s)
        assert b % 256 == 0, (n, s, b)   # the end offset of a carve
        # the two valid planes and the two kept lists on top of the unmasked render's buffers
        assert b >= lib.rdrf_render_workspace_bytes(n, s) + n * s * (2 + 2 * 4), (n, s)
    for s in Ss:
        col = [size[(n, s)] for n in Ns]
        assert col == sorted(col), s
    for n in Ns:
        row = [size[(n, s)] for s in Ss]
        assert row == sorted(row), n


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("c++filt") is None, reason="needs hipcc")
def test_masked_render_kernels_do_not_spill():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    rows = kr.table(os.path.join(kr.CSRC, "rdrf_render_masked.hip"))
    seen = set()
    for r in rows:
        name = subprocess.run(["c++filt", r["name"]], capture_output=True, text=True).stdout.strip()
        seen.add(re.sub(r"^void ", "", re.sub(r"[<(].*", "", name)))
        assert int(r["VGPRs"]) <= 256, (name, r["VGPRs"])
        assert int(r["VGPRs Spill"]) == 0, (name, r["VGPRs Spill"])
        assert int(r["ScratchSize [bytes/lane]"]) == 0, (name, r["ScratchSize [bytes/lane]"])
        assert int(r["Occupancy [waves/SIMD]"]) >= 2, (name, r["Occupancy [waves/SIMD]"])
    assert {"k_keep", "k_static_density_list", "k_static_scan", "k_dyn_density_list"} <= seen, seen
