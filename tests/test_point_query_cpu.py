"""CPU-side checks of the point queries (csrc/rdrf_point.hip, fields.TensorBase.query_points): the two C entry points on
every layer of the boundary, the workspace size against the carve of the launch, and the float64 per-point reference of
tests/_point_prim.py against the reference-generated goldens on their own sample points."""
import ctypes as C
import os
import re

import pytest
import torch

from _point_prim import golden_points, point_reference, ray_norm_viewdirs
from _util import assert_close, load_case, pkg
from oracle import rodynrf_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POINT_CASES = ["ndc_relu", "ndc_softplus", "contract_relu_te", "contract_softplus_te"]
# app-masked samples (golden weight > 1e-4) per case: (static, dynamic, samples)
MASKED = {"ndc_relu": (164, 74, 416), "ndc_softplus": (112, 115, 208), "contract_relu_te": (89, 118, 224),
          "contract_softplus_te": (57, 52, 156)}


def test_symbols_on_every_layer():
    L = pkg()
    hdr = open(os.path.join(ROOT, "include", "rodynrf.h")).read()
    names = ["rdrf_query_points_ws_bytes", "rdrf_query_points"]
    for name in names:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in L.SIGNATURES and hasattr(L.lib, name), name
    order = list(L.SIGNATURES)
    assert order.index(names[1]) == order.index(names[0]) + 1 == order.index("rdrf_render_masked_fwd") + 2
    assert L.lib.rdrf_abi_version() == L.ABI_VERSION == 6
    m = re.search(r"#define\s+RDRF_QUERY_POINTS_MAX\s+\(1 << (\d+)\)", hdr)
    assert m and 1 << int(m.group(1)) == L.QUERY_POINTS_MAX
    assert L.QUERY_POINTS_MAX * 32 + 31 < 2 ** 31   # n * 32 + o of the time branch, the largest int index of the path


@pytest.mark.parametrize("dynamic", [0, 1])
@pytest.mark.parametrize("per_point", [0, 1])
def test_workspace_size_is_the_carve(dynamic, per_point):
    """non-decreasing in M, whole 256-byte blocks, and exactly what the launch demands: with one byte less the entry point
    returns the workspace code.  That check precedes every dereference and every launch, so it runs without a device."""
    L = pkg()
    size = lambda M: L.lib.rdrf_query_points_ws_bytes(dynamic, M, per_point)
    Ms = [0, 1, 31, 32, 33, 165, 4096, 65536, 1 << 20, L.QUERY_POINTS_MAX]
    sizes = [size(M) for M in Ms]
    assert all(s > 0 and s % 256 == 0 for s in sizes)
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[1]
    buf = (C.c_char * 64)()   # stands in for every pointer: the size check comes first and nothing is read
    p = C.addressof(buf)
    for M in (1, 33, 4096):
        rc = L.lib.rdrf_query_points(p, dynamic, p, p, M, p, per_point, p, p, p, p if dynamic else None, p if dynamic else None,
                                     p, size(M) - 1, None)
        assert rc == -3 and b"workspace too small" in L.lib.rdrf_last_error(), (rc, L.lib.rdrf_last_error())
    assert L.lib.rdrf_query_points(p, dynamic, p, p, 0, p, per_point, p, p, p, None, None, None, 0, None) == 0   # M = 0: a no-op
    rc = L.lib.rdrf_query_points(p, dynamic, p, p, L.QUERY_POINTS_MAX + 1, p, per_point, p, p, p, None, None, p, 1 << 40, None)
    assert rc == -1 and b"RDRF_QUERY_POINTS_MAX" in L.lib.rdrf_last_error()


@pytest.mark.parametrize("case", POINT_CASES)
def test_reference_matches_the_goldens_on_their_samples(case):
    """sigma, blending and rgb of the float64 per-point reference at the golden's app-masked samples (weight > 1e-4: where the
    reference computed a colour) against the golden arrays, at the tolerance tests/test_oracle_golden.py holds the oracle's
    forward to for the same arrays (1e-4 of each array's max)."""
    g, sd_s, cfg_s, sd_d, cfg_d = load_case(case)
    rt = str(g["meta.ray_type"])
    xyz, t, vd = golden_points(g, rt)
    valid = torch.from_numpy(g["valid"]).reshape(-1)
    n_s, n_d, n = MASKED[case]
    for tag, sd, cfg, dynamic, want in (("fs.", sd_s, cfg_s, False, n_s), ("fd.", sd_d, cfg_d, True, n_d)):
        m = (torch.from_numpy(g[tag + "weight"]) > 1e-4).reshape(-1)
        assert m.numel() == n and int(m.sum()) == want >= 50, (case, tag, int(m.sum()), m.numel())
        assert bool(valid[m].all())
        ref = point_reference(sd, cfg, xyz[m], t[m], vd[m], dynamic)
        names = ("sigma", "blending", "rgb") if dynamic else ("sigma", "rgb")
        for k in names:
            gold = torch.from_numpy(g[tag + k]).reshape((-1, 3) if k == "rgb" else (-1,))[m]
            assert_close(ref[k], gold, f"{tag}{k}")
        if dynamic:   # every valid sample has an xyz_prime
            full = point_reference(sd, cfg, xyz[valid], t[valid], vd[valid], True)
            assert_close(full["xyz_prime"], torch.from_numpy(g["fd.xyz_prime"]).reshape(-1, 3)[valid], "fd.xyz_prime")


def test_ray_norm_viewdirs_are_unit_and_close_to_torch():
    """the bit-level restatement of ray_norm used by the GPU identity test: within an ulp of the plain quotient"""
    g = load_case("ndc_relu")[0]
    rays = torch.from_numpy(g["rays"])
    vd = ray_norm_viewdirs(rays)
    _, ref = O._dists_viewdirs(rays.double(), torch.from_numpy(g["z"]).double(), "ndc")
    assert float((vd.double() - ref).abs().max()) <= 2.0 ** -23
    assert float((vd.double().norm(dim=-1) - 1).abs().max()) <= 2.0 ** -22
