"""CPU-side tests of the mesh simplification layer: the numpy restatement of vertex clustering (tests/_simplify_prim.py) on
hand-written cases, the edge balance of a clustered closed mesh, idempotence, every refusal of the three C entry points
(argument checks that return before any launch, so they run without a GPU) and the unit's compile check."""
import ctypes as C
import importlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import _simplify_prim as S

from _util import pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = pkg()

_dummy = (C.c_char * 256)()
PTR = C.addressof(_dummy)


# ---- the restatement on hand-written cases -------------------------------------------------------------------------------
def test_two_triangles_sharing_a_cell():
    # lattice 2 x 2 x 1 of unit cells; A and B share cell (0,0); keys: (0,0) 0, (0,1) 1, (1,0) 2, (1,1) 3
    A, B, Cc, D, E = [0.25, 0.25, 0.5], [0.75, 0.25, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [1.5, 1.5, 0.5]
    verts = np.array([A, B, Cc, D, E], dtype=np.float32)
    faces = np.array([[0, 2, 3], [1, 4, 3]])
    colors = np.array([[0, 1, 255], [1, 2, 254], [9, 9, 9], [7, 7, 7], [5, 5, 5]], dtype=np.uint8)
    m = S.simplify(verts, faces, [0, 0, 0], [1, 1, 1], [2, 2, 1], colors=colors)
    assert m["counts"] == (4, 2)
    assert np.array_equal(m["verts"], np.array([[0.5, 0.25, 0.5], D, Cc, E], dtype=np.float32))
    assert np.array_equal(m["faces"], [[0, 2, 1], [0, 3, 1]])          # order and winding kept
    assert np.array_equal(m["remap"], [0, 0, 2, 1, 3])
    assert np.array_equal(m["colors"], [[1, 2, 255], [7, 7, 7], [9, 9, 9], [5, 5, 5]])   # means 0.5, 1.5, 254.5 round half up
    assert np.array_equal(m["k"], [2, 1, 1, 1])


def test_a_fan_inside_one_cell_collapses_to_nothing():
    rng = np.random.default_rng(0)
    verts = rng.uniform(0.1, 0.9, (7, 3)).astype(np.float32)
    faces = np.array([[0, i, i + 1] for i in range(1, 6)])
    m = S.simplify(verts, faces, [0, 0, 0], [1, 1, 1], [3, 3, 3])
    assert m["counts"] == (0, 0) and len(m["verts"]) == 0 and len(m["faces"]) == 0 and (m["remap"] == -1).all()
    m = S.simplify(verts, faces, [0, 0, 0], [1, 1, 1], [3, 3, 3], drop_unreferenced=False)
    assert m["counts"] == (1, 0) and (m["remap"] == 0).all()
    assert np.allclose(m["verts"][0], verts.astype(np.float64).mean(0), rtol=0, atol=2.0 ** -24)


def test_boundaries_outside_and_nan():
    one = np.float32(1.5)
    below = np.nextafter(one, np.float32(0))
    verts = np.array([[one, 0, 0], [below, 0, 0], [-5.0, 0, 0], [100.0, 0, 0], [np.nan, 0.75, 0], [0.25, np.inf, -np.inf], [0, 0, 1.0]],
                     dtype=np.float32)
    c = S.cells(verts, [0, 0, 0], [0.5, 0.5, 0.5], [4, 2, 2])
    assert c[0, 0] == 3 and c[1, 0] == 2            # dyadic: (1.5 - 0) / 0.5 is exactly 3, floor decides
    assert c[2, 0] == 0 and c[3, 0] == 3            # outside on both sides: clamped
    assert c[4].tolist() == [0, 1, 0]               # NaN: cell 0 on that axis
    assert c[5].tolist() == [0, 1, 0]               # +inf clamps to the top, -inf to 0
    assert c[6].tolist() == [0, 0, 1]               # the last cell is closed above: 1.0 / 0.5 = 2 clamps to n - 1
    assert S.keys_of(verts, [0, 0, 0], [0.5, 0.5, 0.5], [4, 2, 2]).tolist() == [12, 8, 0, 12, 2, 2, 1]
    # topology and counts still hold with a NaN member
    m = S.simplify(verts, [[0, 1, 2], [4, 5, 6], [2, 6, 4], [0, 9, 1]], [0, 0, 0], [0.5, 0.5, 0.5], [4, 2, 2])
    # clusters by key: {2}, {6}, {4, 5}, {1}, {0, 3}; face [4,5,6]: 4 and 5 share a cluster; [0,9,1]: index 9 is out of range
    assert m["counts"] == (5, 2) and np.array_equal(m["faces"], [[4, 3, 0], [0, 1, 2]])
    assert np.array_equal(m["remap"], [4, 3, 0, 4, 2, 2, 1])
    assert S.simplify(verts[:0], np.zeros((0, 3)), [0, 0, 0], [1, 1, 1], [1, 1, 1])["counts"] == (0, 0)
    assert S.simplify(verts, np.zeros((0, 3)), [0, 0, 0], [1, 1, 1], [1, 1, 1], drop_unreferenced=False)["counts"] == (0, 0)


# ---- properties ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["capped_ball", "torus", "sphere", "two_spheres"])
def test_edge_balance_of_clustered_closed_meshes(name):
    """clustering is a simplicial map and degenerate faces map to nothing: on a closed oriented input every directed edge
    a -> b of the output occurs exactly as often as b -> a"""
    verts, faces, aabb, shape, cap = S.closed_meshes()[name]
    assert S.unbalanced_edges(faces) == 0 and len(faces) > 500
    assert S.unbalanced_edges(faces[:-1]) > 0                      # the helper sees an open mesh
    for K in (2, 3, 5):
        origin, cell, n = S.lattice(aabb, shape, K, cap)
        m = S.simplify(verts, faces, origin, cell, n)
        nv, nf = m["counts"]
        print(f"{name} K={K}: {len(verts)} -> {nv} vertices, {len(faces)} -> {nf} faces")
        assert 0 < nv < len(verts) and 0 < nf < len(faces)
        assert S.unbalanced_edges(m["faces"]) == 0
        f = m["faces"]
        assert (f[:, 0] != f[:, 1]).all() and (f[:, 1] != f[:, 2]).all() and (f[:, 0] != f[:, 2]).all()
        assert np.array_equal(np.unique(f), np.arange(nv))          # every vertex is referenced
        # every representative lies in the closed box of its cell
        c = S.cells(m["verts"], origin, cell, n)
        key = (c[:, 0] * n[1] + c[:, 1]) * n[2] + c[:, 2]
        assert (np.diff(key) > 0).all()                             # ascending keys, one vertex per cell
        # idempotence: the same lattice again changes nothing
        again = S.simplify(m["verts"], m["faces"], origin, cell, n)
        assert again["verts"].tobytes() == m["verts"].tobytes() and np.array_equal(again["faces"], m["faces"])
        assert np.array_equal(again["remap"], np.arange(nv))


def dyadic_mesh(rng, V, F, span=4.0):
    verts = (rng.integers(-int(span * 64), int(span * 64), (V, 3)) / 64.0).astype(np.float32)
    return verts, rng.integers(0, V, (F, 3))


def test_idempotence_on_dyadic_inputs():
    rng = np.random.default_rng(11)
    verts, faces = dyadic_mesh(rng, 700, 2000)
    nrm = rng.standard_normal((700, 3)).astype(np.float32)
    col = rng.integers(0, 256, (700, 3)).astype(np.uint8)
    for cell, n in (([0.5, 0.25, 1.0], [16, 32, 8]), ([1.0, 1.0, 1.0], [5, 9, 8])):   # the second clamps on the first axis
        m = S.simplify(verts, faces, [-4, -4, -4], cell, n, normals=nrm, colors=col)
        assert 0 < m["counts"][0] < 700 and 0 < m["counts"][1] < 2000
        again = S.simplify(m["verts"], m["faces"], [-4, -4, -4], cell, n, normals=m["normals"], colors=m["colors"])
        assert again["verts"].tobytes() == m["verts"].tobytes() and np.array_equal(again["faces"], m["faces"])
        assert np.array_equal(again["colors"], m["colors"])
        assert np.abs(again["normals"].astype(np.float64) - m["normals"]).max() <= 2.0 ** -23   # renormalising a rounded unit vector


def test_general_case_of_the_gpu_test_stays_within_its_boundary_cap():
    """tests/test_gpu_simplify.py::test_general_inputs leaves out the vertices within one fp32 rounding of a cell boundary and
    fails above 1 % of the batch: its seed keeps the restatement alone within that cap, and its vertices reach every clamp"""
    import test_gpu_simplify as G
    verts = G.general_case()[0]
    assert G.near_a_boundary(verts).sum() <= G.GEN_V // 100
    c = S.cells(verts, G.GEN_ORIGIN, G.GEN_CELL, G.GEN_N)
    assert (c.min(0) == 0).all() and (c.max(0) == np.array(G.GEN_N) - 1).all()
    k = np.bincount(S.keys_of(verts, G.GEN_ORIGIN, G.GEN_CELL, G.GEN_N))
    assert (k > 0).sum() > 1000 and k.max() > 20


# ---- the three entry points' refusals, through the library -------------------------------------------------------------------
def i3(*v):
    return (C.c_int * 3)(*v)


def f3(*v):
    return (C.c_float * 3)(*v)


def count(V=5, F=7, n=(4, 4, 4), origin=(0, 0, 0), cell=(1, 1, 1), verts=PTR, faces=PTR, ws=PTR, ws_bytes=None, counts=PTR):
    nn = None if n is None else i3(*n)
    if ws_bytes is None:
        ws_bytes = L.lib.rdrf_simplify_ws_bytes(V, F, nn)
    rc = L.lib.rdrf_simplify_count(verts, V, faces, F, None if origin is None else f3(*origin), None if cell is None else f3(*cell), nn, 1,
                                   ws, ws_bytes, counts, None, None)
    return rc, L.lib.rdrf_last_error().decode()


def emit(V=5, F=7, nv=3, nf=2, verts=PTR, faces=PTR, ws=PTR, verts_out=PTR, faces_out=PTR, normals=None, normals_out=None, colors=None,
         colors_out=None):
    rc = L.lib.rdrf_simplify_emit(verts, normals, colors, V, faces, F, ws, verts_out, normals_out, colors_out, faces_out, nv, nf, None)
    return rc, L.lib.rdrf_last_error().decode()


def test_header_and_binding():
    hdr = open(os.path.join(ROOT, "include", "rodynrf.h")).read()
    order = re.findall(r"^\s*(?:size_t|int)\s+(rdrf_\w+)\s*\(", hdr, flags=re.M)
    names = ["rdrf_simplify_ws_bytes", "rdrf_simplify_count", "rdrf_simplify_emit"]
    at = order.index("rdrf_query_points")
    assert order[at + 1:at + 4] == names
    keys = list(L.SIGNATURES)
    assert keys[keys.index("rdrf_query_points") + 1:][:3] == names
    for name in names:
        assert hasattr(L.lib, name), name
    assert len(L.SIGNATURES["rdrf_simplify_count"][1]) == 13 and len(L.SIGNATURES["rdrf_simplify_emit"][1]) == 14
    import rodynrf
    for name in ("simplify_mesh", "simplify_lattice"):
        assert name in rodynrf.__all__ and hasattr(rodynrf, name), name


def test_size_function_and_its_refusals():
    size = lambda V, F, n: L.lib.rdrf_simplify_ws_bytes(V, F, None if n is None else i3(*n))
    for V, F, n in ((-1, 5, (2, 2, 2)), (5, -1, (2, 2, 2)), (2 ** 31, 5, (2, 2, 2)), (5, 2 ** 31, (2, 2, 2)), (5, 5, (0, 2, 2)), (5, 5, (2, -1, 2)),
                    (5, 5, (2, 2, 0)), (5, 5, (2048, 1024, 1024)), (5, 5, (65536, 65536, 65536)), (5, 5, None)):
        assert size(V, F, n) == 0, (V, F, n)
    assert size(5, 5, (2047, 1024, 1024)) > 0 and size(0, 0, (1, 1, 1)) > 0 and size(2 ** 31 - 1, 2 ** 31 - 1, (1, 1, 1)) > 2 ** 31 * 30
    V, F = 100000, 200000
    need = size(V, F, (8, 8, 8))
    assert need % 256 == 0 and need == size(V, F, (1290, 1290, 1290))    # the layout does not depend on the lattice
    # keys, sorted keys, order, cluster, start (5 x 4 V), marks + two local prefixes (3 V), the faces' local prefix (F), the sort
    assert 23 * V + F <= need <= 23 * V + F + L.lib.rdrf_selftest_sort_temp_bytes(V, 32) + 64 * 256 + 3 * 4 * (V // 256 + F // 256)
    assert size(V + 1, F, (8, 8, 8)) >= need and size(V, F + 1, (8, 8, 8)) >= need


def test_count_refusals_return_before_any_launch():
    """null or dummy pointers throughout: a call that got as far as a launch would fail; these return from the argument checks"""
    assert count(V=-1) == (-1, "simplify_count: negative counts (-1 vertices, 7 faces)")
    assert count(F=-2) == (-1, "simplify_count: negative counts (5 vertices, -2 faces)")
    assert count(V=2 ** 31) == (-1, "simplify_count: 2147483648 vertices, the vertex indices are 32-bit ints (at most 2147483647)")
    assert count(F=2 ** 31) == (-1, "simplify_count: 2147483648 faces, the face prefixes are 32-bit (at most 2147483647)")
    assert count(n=None) == (-1, "simplify_count: no lattice")
    for n in ((0, 4, 4), (4, 0, 4), (4, 4, -1)):
        assert count(n=n) == (-1, f"simplify_count: every side of the lattice must have at least 1 cell, not {n[0]} x {n[1]} x {n[2]}")
    assert count(n=(2048, 1024, 1024)) == (-1, "simplify_count: 2048 x 1024 x 1024 has 2147483648 cells, the keys are below 2^31")
    rc, msg = count(n=(2 ** 30, 2 ** 30, 2 ** 30))      # the product overflows 64 bits as an integer: refused, not wrapped
    assert rc == -1 and "cells" in msg, (rc, msg)
    assert count(origin=None) == (-1, "simplify_count: no lattice origin or cell size")
    assert count(cell=None) == (-1, "simplify_count: no lattice origin or cell size")
    for cell in ((0, 1, 1), (1, -1, 1), (1, 1, float("inf")), (float("nan"), 1, 1)):
        rc, msg = count(cell=cell)
        assert rc == -1 and msg.startswith("simplify_count: cell sizes must be positive and finite, not "), (cell, rc, msg)
    rc, msg = count(origin=(0, float("nan"), 0))
    assert rc == -1 and msg.startswith("simplify_count: the origin must be finite, not "), (rc, msg)
    assert count(counts=None) == (-1, "simplify_count: bad arguments")
    assert count(verts=None) == (-1, "simplify_count: bad arguments")
    assert count(faces=None) == (-1, "simplify_count: bad arguments")
    assert count(ws=None) == (-3, "simplify_count: no workspace")
    need = L.lib.rdrf_simplify_ws_bytes(5, 7, i3(4, 4, 4))
    assert count(ws_bytes=need - 1) == (-3, f"simplify_count: workspace too small: need {need} have {need - 1}")
    assert count(ws_bytes=0) == (-3, f"simplify_count: workspace too small: need {need} have 0")


def test_emit_refusals_return_before_any_launch():
    assert emit(V=-1) == (-1, "simplify_emit: negative counts (-1 vertices, 7 faces)")
    assert emit(V=2 ** 31, nv=0) == (-1, "simplify_emit: 2147483648 vertices, the vertex indices are 32-bit ints (at most 2147483647)")
    assert emit(F=2 ** 31) == (-1, "simplify_emit: 2147483648 faces, the face prefixes are 32-bit (at most 2147483647)")
    assert emit(nv=6) == (-1, "simplify_emit: 6 vertices and 2 faces out of 5 and 7")
    assert emit(nf=8) == (-1, "simplify_emit: 3 vertices and 8 faces out of 5 and 7")
    assert emit(nv=-1) == (-1, "simplify_emit: -1 vertices and 2 faces out of 5 and 7")
    assert emit(nv=0, nf=0, verts=None, faces=None, ws=None)[0] == 0          # an empty result: no launch, nothing read
    assert emit(V=0, F=0, nv=0, nf=0, ws=None)[0] == 0
    for kw in (dict(verts=None), dict(faces=None), dict(verts_out=None), dict(faces_out=None)):
        assert emit(**kw) == (-1, "simplify_emit: bad arguments"), kw
    for kw in (dict(normals=PTR), dict(normals_out=PTR), dict(colors=PTR), dict(colors_out=PTR)):
        assert emit(**kw) == (-1, "simplify_emit: normals and colours need both their input and their output"), kw
    assert emit(ws=None) == (-3, "simplify_emit: no workspace")


def test_python_surface_refuses_by_name():
    import rodynrf
    v, f = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32)
    with pytest.raises(rodynrf.RdrfError, match="CPU tensor"):
        rodynrf.simplify_mesh(v, f, cell=1.0)
    for K in (0, -1, 1.5, True, "2"):
        with pytest.raises(rodynrf.RdrfError, match="simplify must be a whole number"):
            rodynrf.simplify_lattice([0, 0, 0, 1, 1, 1], (5, 5, 5), K)
        with pytest.raises(rodynrf.RdrfError, match="simplify must be a whole number"):
            rodynrf.mesh_sequence(None, [0.0], simplify=K)
    lat = rodynrf.simplify_lattice([-1, -1, -1, 1, 1, 3], (9, 10, 11), 3)
    assert lat["grid"] == [3, 3, 4] and np.allclose(lat["cell"], [0.75, 2 / 3, 1.2]) and lat["aabb"].tolist() == [-1, -1, -1, 1, 1, 3]
    o, c, n = S.lattice([[-1, -1, -1], [1, 1, 3]], (9, 10, 11), 3)
    assert n == lat["grid"] and np.array_equal(np.float32(lat["cell"]), c) and np.array_equal(lat["aabb"][:3].numpy(), o)
    lat = rodynrf.simplify_lattice([-1, -1, -1, 1, 1, 3], (9, 10, 11), 2, cap=True)
    o, c, n = S.lattice([[-1, -1, -1], [1, 1, 3]], (9, 10, 11), 2, cap=True)
    assert n == lat["grid"] == [5, 6, 6] and np.array_equal(np.float32(lat["cell"]), c) and np.array_equal(lat["aabb"][:3].numpy(), o)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("c++filt") is None, reason="needs hipcc")
def test_simplification_kernels_use_no_scratch():
    """the object-file inspection of tests/test_kernel_resources_cpu.py on csrc/rdrf_simplify.hip: no spills, no scratch"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    seen = set()
    for r in kr.table(os.path.join(kr.CSRC, "rdrf_simplify.hip")):
        name = subprocess.run(["c++filt", r["name"]], capture_output=True, text=True).stdout.strip()
        seen.add(re.sub(r"\(.*", "", name))
        assert int(r["VGPRs Spill"]) == 0 and int(r["ScratchSize [bytes/lane]"]) == 0, (name, r)
        assert int(r["VGPRs"]) <= 64, (name, r["VGPRs"])          # eight waves per SIMD
    assert seen == {"k_simp_keys", "k_simp_heads", "k_simp_scan", "k_simp_assign", "k_simp_fcount", "k_simp_used", "k_simp_remap",
                    "k_simp_verts", "k_simp_faces"}, seen
    src = open(os.path.join(kr.CSRC, "rdrf_simplify.hip")).read()
    assert "atomic" not in re.sub(r"//[^\n]*", "", src)             # no atomics anywhere in the unit (the sort's are on LDS)
