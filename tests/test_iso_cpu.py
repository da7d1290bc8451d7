"""CPU-side tests of the isosurface layer: the float64 restatement of marching tetrahedra (tests/_iso_prim.py) on analytic
volumes and on every sign pattern of a cube and of a pair of cubes, the PLY writer / reader, the three C prototypes and the
size refusals of rdrf_iso_count (argument checks that return before any launch, so they run without a GPU)."""
import ctypes as C
import importlib
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import _iso_prim as P

from _util import pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT = [[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]]


@pytest.mark.parametrize("name", ["sphere", "torus", "two_spheres"])
def test_restatement_on_analytic_volumes(name):
    vol, chi, analytic = P.analytic_cases()[name]
    m = P.reference(name)
    assert len(m["verts"]) > 500 and len(m["faces"]) > 1000
    assert P.is_closed(m["faces"]) and P.is_oriented(m["faces"])
    assert P.euler_characteristic(len(m["verts"]), m["faces"]) == chi
    vol_mesh = P.signed_volume(m["verts"], m["faces"])
    print(f"{name}: V = {vol_mesh:.5f}, analytic {analytic:.5f}")
    assert vol_mesh > 0 and abs(vol_mesh - analytic) < 0.05 * analytic   # a 24^3 lattice: a few percent inside the surface
    assert P.signed_volume(m["verts"], P.marching_tets(vol, 0.0, P.AABB, flip=True)["faces"]) == -vol_mesh
    # every vertex lies on its edge and on the level set of the edge's linear interpolant
    assert (m["t"] > 0).all() and (m["t"] <= 1).all()
    # the normals of the GPU test: at most 1 % of the vertices fall under the gradient floor (none here), unit length
    low = m["gnorm"] < P.GRADIENT_FLOOR * m["gscale"]
    assert low.mean() <= 0.01, low.mean()
    assert np.allclose(np.linalg.norm(m["normals"][~low], axis=1), 1.0, atol=1e-12)
    # -grad v points to lower values, as the face normals do: the vertex normal agrees with every face around it
    fn = np.cross(m["verts"][m["faces"][:, 1]] - m["verts"][m["faces"][:, 0]], m["verts"][m["faces"][:, 2]] - m["verts"][m["faces"][:, 0]])
    agree = np.einsum("ij,ij->i", fn, m["normals"][m["faces"][:, 0]])
    assert (agree > 0).mean() > 0.99


def test_all_256_sign_patterns_of_one_cube():
    rng = np.random.default_rng(256)
    tet_edges = P.tet_edge_set()
    for pattern, vol in enumerate(P.all_sign_patterns(rng)):
        m = P.marching_tets(vol, 0.5, UNIT)
        inside = [(pattern >> c) & 1 for c in range(8)]
        # every crossed edge of the 19 has exactly one vertex
        crossed = set()
        for code in range(8):
            for kind in range(7):
                up = code + kind + 1
                if (code & (kind + 1)) == 0 and up < 8 and inside[code] != inside[up]:
                    crossed.add((code, kind))   # (2,2,2): a point's linear index is its corner code
        keys = [tuple(k) for k in m["keys"].tolist()]
        assert len(keys) == len(set(keys)) and set(keys) == crossed and keys == sorted(keys), pattern
        # the triangle count is the sum over the tetrahedra of 0, 1 or 2
        want = 0
        for q in range(6):
            n_in = sum(inside[c] for c in P.tet_corner_codes(q))
            want += {0: 0, 1: 1, 2: 2, 3: 1, 4: 0}[n_in]
        assert len(m["faces"]) == want, pattern
        # every triangle's three vertices lie on edges of one tetrahedron
        for f in m["faces"].tolist():
            tri = {keys[i] for i in f}
            assert len(tri) == 3 and any(tri <= edges for edges in tet_edges), (pattern, f)


def test_adjacent_cubes_agree_on_the_shared_face():
    """a 3 x 2 x 2 block is two cubes that share the face i = 1; for every sign pattern of its twelve corners (every pair of
    adjacent cube patterns) the mesh edges lying in that face are used once in each direction: what one cube's patch leaves
    open there the other closes.  Watertightness across cubes, checked instead of assumed."""
    rng = np.random.default_rng(12)
    mag = rng.uniform(0.05, 0.45, (3, 2, 2)).astype(np.float32)
    seen_face_edges = 0
    for pattern in range(1 << 12):
        bits = np.array([(pattern >> b) & 1 for b in range(12)]).reshape(3, 2, 2)
        vol = np.float32(0.5) + np.where(bits == 1, mag, -mag)
        m = P.marching_tets(vol, 0.5, [[0, 0, 0], [2, 1, 1]])
        if len(m["faces"]) == 0:
            continue
        on_face = (m["ends"][:, :, 0] == 1).all(1)   # both ends of the vertex's lattice edge on the plane i = 1
        d = P.directed_edge_counts(m["faces"])
        for (a, b), n in d.items():
            assert n == 1, pattern
            if on_face[a] and on_face[b]:
                seen_face_edges += 1
                assert d.get((b, a), 0) == 1, (pattern, a, b)
    assert seen_face_edges > 4096


@pytest.mark.parametrize("with_normals,with_colors", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("nv", [0, 7])
def test_ply_round_trip_is_bit_exact(tmp_path, nv, with_normals, with_colors):
    import rodynrf
    rng = np.random.default_rng(nv)
    verts = rng.standard_normal((nv, 3)).astype(np.float32)
    if nv:
        verts[0, 0] = np.float32(-0.0)
        verts[1, 1] = np.nextafter(np.float32(1), np.float32(2))
    faces = rng.integers(0, max(nv, 1), (0 if nv == 0 else 11, 3)).astype(np.int32)
    normals = rng.standard_normal((nv, 3)).astype(np.float32) if with_normals else None
    colors = rng.integers(0, 256, (nv, 3)).astype(np.uint8) if with_colors else None
    path = str(tmp_path / "m.ply")
    rodynrf.write_ply(path, torch.from_numpy(verts), torch.from_numpy(faces), normals, colors)
    head = open(path, "rb").read(200)
    assert head.startswith(b"ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\n" % nv)
    back = rodynrf.read_ply(path)
    assert back["verts"].dtype == np.float32 and back["verts"].tobytes() == verts.tobytes() and back["verts"].shape == (nv, 3)
    assert back["faces"].dtype == np.int32 and np.array_equal(back["faces"], faces) and back["faces"].shape == faces.shape
    for got, want in ((back["normals"], normals), (back["colors"], colors)):
        assert (got is None) == (want is None)
        if want is not None:
            assert got.dtype == want.dtype and got.tobytes() == want.tobytes()
    expect = len(head[:head.index(b"end_header\n")]) + len(b"end_header\n") if b"end_header\n" in head else None
    if expect is not None:
        assert os.path.getsize(path) == expect + nv * (12 + 12 * with_normals + 3 * with_colors) + len(faces) * 13


def test_header_and_binding():
    L = pkg()
    hdr = open(os.path.join(ROOT, "include", "rodynrf.h")).read()
    order = re.findall(r"^\s*(?:size_t|int)\s+(rdrf_\w+)\s*\(", hdr, flags=re.M)
    names = ["rdrf_iso_ws_bytes", "rdrf_iso_count", "rdrf_iso_emit"]
    at = order.index("rdrf_alpha_mask_valid")
    assert order[at + 1:at + 4] == names                      # appended to the alpha-mask block
    keys = list(L.SIGNATURES)
    assert keys[keys.index("rdrf_alpha_mask_valid") + 1:][:3] == names
    for n in names:
        assert hasattr(L.lib, n), n
    assert L.SIGNATURES["rdrf_iso_count"] == (C.c_int, [C.c_void_p] + [C.c_int] * 5 + [C.c_float, C.c_void_p, C.c_size_t, C.c_void_p,
                                                                                    C.c_void_p])
    assert len(L.SIGNATURES["rdrf_iso_emit"][1]) == 16
    assert L.lib.rdrf_abi_version() == L.ABI_VERSION == 6
    assert "#define RDRF_ABI_VERSION 6" in hdr


def test_size_refusals_return_before_any_launch():
    """null volume, workspace and counts: a call that got as far as a launch would fault; these return from the argument checks"""
    L = pkg()

    def count(G, T=1, t=0):
        rc = L.lib.rdrf_iso_count(None, G[0], G[1], G[2], T, t, 0.5, None, 0, None, None)
        return rc, L.lib.rdrf_last_error().decode()

    for G in ((1, 2, 2), (2, 1, 2), (2, 2, 1), (0, 5, 5), (-3, 5, 5)):
        rc, msg = count(G)
        assert rc == -1 and "at least 2" in msg, (G, rc, msg)
        assert L.lib.rdrf_iso_ws_bytes(*G) == 0
    rc, msg = count((675, 675, 675))        # 7 x 307 546 875 >= 2^31
    assert rc == -1 and "possible vertices" in msg, (rc, msg)
    rc, msg = count((670, 670, 670))        # 7 x 300 763 000 < 2^31 <= 12 x 669^3
    assert rc == -1 and "possible triangles" in msg, (rc, msg)
    assert L.lib.rdrf_iso_ws_bytes(675, 675, 675) == 0 and L.lib.rdrf_iso_ws_bytes(670, 670, 670) == 0
    rc, msg = count((2048, 2048, 2048))     # the products overflow 32 bits: refused, not wrapped
    assert rc == -1, (rc, msg)
    rc, msg = count((500, 500, 500))        # inside both limits: the next check (no workspace) speaks
    assert rc == -3 and "workspace" in msg, (rc, msg)
    rc, msg = count((5, 5, 5), T=3, t=3)
    assert rc == -1 and "slice" in msg, (rc, msg)
    n = 24 * 24 * 24
    need = L.lib.rdrf_iso_ws_bytes(24, 24, 24)
    assert need % 256 == 0 and 5 * n <= need <= 5 * n + 8 * (n // 256 + 1) + 5 * 256 + 3 * 256   # flags + local prefix + three sum tables
    rc, msg = L.lib.rdrf_iso_count(None, 24, 24, 24, 1, 0, 0.5, C.c_void_p(256), need - 1, None, None), L.lib.rdrf_last_error().decode()
    assert rc == -3 and "too small" in msg, (rc, msg)


def test_cpu_tensors_are_refused():
    import rodynrf
    with pytest.raises(rodynrf.RdrfError):
        rodynrf.extract_isosurface(torch.zeros(4, 4, 4), 0.5, UNIT)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("c++filt") is None, reason="needs hipcc")
def test_isosurface_kernels_use_no_scratch():
    """the object-file inspection of tests/test_kernel_resources_cpu.py on csrc/rdrf_iso.hip: no spills, no scratch"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    seen = set()
    for r in kr.table(os.path.join(kr.CSRC, "rdrf_iso.hip")):
        name = subprocess.run(["c++filt", r["name"]], capture_output=True, text=True).stdout.strip()
        seen.add(re.sub(r"\(.*", "", name))
        assert int(r["VGPRs Spill"]) == 0 and int(r["ScratchSize [bytes/lane]"]) == 0, (name, r)
        assert int(r["VGPRs"]) <= 64, (name, r["VGPRs"])          # eight waves per SIMD
    assert seen == {"k_iso_count", "k_iso_scan", "k_iso_verts", "k_iso_faces"}, seen
