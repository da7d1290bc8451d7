"""CPU tests of the texture atlas (mesh.atlas_layout / atlas_uv / write_obj / read_obj, tests/_bake_prim.py): the layout and
the texture coordinates against the float64 reference, ownership, the footprint of a bilinear fetch inside every face, the
OBJ + MTL + PNG round trip, the written bound on a float32 evaluation in the kernel's order, and the argument errors that are
raised before any device work."""
import os
import struct
import zlib

import numpy as np
import pytest
import torch

import _bake_prim as B
from _util import pkg, record_margin

M = pkg("mesh")
L = pkg()

QS = (4, 5, 8, 64)


def cases():
    """(F, q, width): F in {0, 1, 2, 3, 2R - 1, 2R, 2R + 1} for widths that leave a ragged right margin, and the default width"""
    out = []
    for q in QS:
        for width in (None, 2 * q + 3, 3 * q + q // 2):
            R = 2 if width is None else width // q
            for F in (0, 1, 2, 3, 2 * R - 1, 2 * R, 2 * R + 1):
                out.append((F, q, width))
    return out


@pytest.mark.parametrize("q", QS)
def test_layout_and_uv_match_the_reference(q):
    for F, qq, width in (c for c in cases() if c[1] == q):
        got = M.atlas_layout(F, q, width)
        assert got == B.layout(F, q, width), (F, q, width)
        Wt, Ht, R = got
        assert R == Wt // q >= 1 and Ht == q * (-(-((F + 1) // 2) // R))
        if width is None:
            need = q * max(1, int(np.ceil(np.sqrt((F + 1) // 2))))
            assert Wt >= need and Wt & (Wt - 1) == 0 and (Wt // 2 < need or Wt == 1)
        uv = M.atlas_uv(F, q, width)
        assert uv.dtype == torch.float32 and tuple(uv.shape) == (F, 3, 2)
        assert np.array_equal(uv.numpy(), B.uv(F, q, width).astype(np.float32)), (F, q, width)
    for F in (7, 200, 45537):   # the default width over a range of sizes
        Wt, Ht, R = M.atlas_layout(F, q)
        assert (Wt, Ht, R) == B.layout(F, q) and R * (Ht // q) >= (F + 1) // 2


@pytest.mark.parametrize("q", QS)
def test_every_texel_has_at_most_one_owner_and_every_face_its_texels(q):
    for F, _, width in (c for c in cases() if c[1] == q):
        Wt, Ht, R = B.layout(F, q, width)
        own = B.ownership(F, q, Wt)
        face = own["face"]
        assert face.shape == (Ht, Wt)
        # the rule, face by face, claims disjoint texel sets: count the claims per texel
        claims = np.zeros((Ht, Wt), dtype=np.int64)
        for f in range(F):
            s = f >> 1
            sx, sy = (s % R) * q, (s // R) * q
            j, i = np.meshgrid(np.arange(q), np.arange(q), indexing="ij")
            mine = (i + j > q - 1) if f & 1 else (i + j <= q - 1)
            claims[sy:sy + q, sx:sx + q] += mine
            assert (face[sy:sy + q, sx:sx + q][mine] == f).all()
            assert int(mine.sum()) == (q * (q - 1) // 2 if f & 1 else q * (q + 1) // 2)
        assert claims.max(initial=0) <= 1 and ((claims == 1) == (face >= 0)).all()
        assert (face[:, R * q:] == -1).all()
        if F & 1:
            s = F >> 1
            sq = face[(s // R) * q:(s // R) * q + q, (s % R) * q:(s % R) * q + q]
            assert (sq[own["upper"][:q, :q]] == -1).all()


@pytest.mark.parametrize("q", QS)
def test_a_bilinear_fetch_inside_a_face_reads_that_face_only(q):
    """the three corners, the three edge midpoints and a lattice of interior points (barycentric weights in eighths: exact in
    float64) of every face; the gutters make it hold without a dilation pass"""
    lattice = [(a / 8.0, b / 8.0) for a in range(9) for b in range(9 - a)]   # corners and edge midpoints among them
    assert (1.0, 0.0) in lattice and (0.5, 0.5) in lattice and (0.0, 0.5) in lattice
    for F, _, width in (c for c in cases() if c[1] == q and c[0] > 0):
        Wt, Ht, _ = B.layout(F, q, width)
        face = B.ownership(F, q, Wt)["face"]
        corners = B.corners_texel(F, q, Wt)
        for f in range(F):
            for w1, w2 in lattice:
                p = (1.0 - w1 - w2) * corners[f, 0] + w1 * corners[f, 1] + w2 * corners[f, 2]
                for x, y in B.footprint(p[0], p[1]):
                    assert 0 <= x < Wt and 0 <= y < Ht and face[y, x] == f, (F, q, width, f, w1, w2, x, y)


def test_gutter_weights():
    """the weights are those of the texel's centre against the local corners; w0 < 0 exactly on the two diagonals"""
    for q in QS:
        j, i = np.meshgrid(np.arange(q), np.arange(q), indexing="ij")
        upper = i + j > q - 1
        w0, w1, w2 = B.weights(q, i, j, upper)
        for up in (False, True):
            c = B.local_corners(q, up)
            centre = w0[..., None] * c[0] + w1[..., None] * c[1] + w2[..., None] * c[2]
            want = np.stack((i + 0.5, j + 0.5), -1)
            assert np.abs(centre - want)[upper == up].max() < 1e-12
        assert ((w0 < -1e-9) == ((i + j == q - 1) | (i + j == q))).all()


def _png_decode(path):
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, head = 8, b"", None
    while pos < len(data):
        n, kind = struct.unpack(">I", data[pos:pos + 4])[0], data[pos + 4:pos + 8]
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(kind + body) & 0xFFFFFFFF, kind
        if kind == b"IHDR":
            head = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat += body
        pos += 12 + n
    assert kind == b"IEND" and head[2:] == (8, 2, 0, 0, 0)   # 8-bit RGB, no interlace
    rows = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(head[1], 1 + head[0] * 3)
    assert not rows[:, 0].any()   # filter 0
    return rows[:, 1:].reshape(head[1], head[0], 3)


@pytest.mark.parametrize("with_normals", [False, True])
def test_obj_round_trip(tmp_path, with_normals):
    rng = np.random.default_rng(4)
    nv, F, q = 9, 5, 4
    verts = rng.standard_normal((nv, 3)).astype(np.float32) * np.float32(3.7)
    verts[0] = [1e-20, -123456.789, 0.1]
    faces = rng.integers(0, nv, (F, 3)).astype(np.int32)
    normals = rng.standard_normal((nv, 3)).astype(np.float32) if with_normals else None
    Wt, Ht, _ = M.atlas_layout(F, q, 11)
    uv = M.atlas_uv(F, q, 11)
    tex = rng.integers(0, 256, (Ht, Wt, 3)).astype(np.uint8)
    path = tmp_path / "mesh.ply"   # any suffix: it is replaced
    out = M.write_obj(str(path), torch.from_numpy(verts), faces, uv, torch.from_numpy(tex), normals=normals)
    assert [os.path.basename(p) for p in out] == ["mesh.obj", "mesh.mtl", "mesh.png"] and all(os.path.exists(p) for p in out)
    assert not path.exists()
    img = _png_decode(out[2])
    assert img.shape == (Ht, Wt, 3) and np.array_equal(img, tex[::-1])   # row y of the array at image row Ht - 1 - y
    mtl = open(out[1]).read().split("\n")
    assert "map_Kd mesh.png" in mtl and any(line.startswith("newmtl ") for line in mtl)
    text = open(out[0]).read().split("\n")
    assert "mtllib mesh.mtl" in text and sum(line.startswith("vt ") for line in text) == 3 * F
    f_lines = [line for line in text if line.startswith("f ")]
    a, b, c = faces[2] + 1
    assert f_lines[2] == (f"f {a}/7/{a} {b}/8/{b} {c}/9/{c}" if with_normals else f"f {a}/7 {b}/8 {c}/9")
    back = M.read_obj(str(tmp_path / "mesh.obj"))
    assert back["verts"].tobytes() == verts.tobytes() and back["faces"].tobytes() == faces.tobytes()
    assert back["uv"].tobytes() == uv.numpy().tobytes() and np.array_equal(back["texture"], tex)
    assert (back["normals"] is None) if normals is None else (back["normals"].tobytes() == normals.tobytes())
    assert "map_Kd mesh.png" in back["mtl"]
    with pytest.raises(L.RdrfError, match="uv must be"):
        M.write_obj(str(path), verts, faces, uv[:-1], tex)
    with pytest.raises(L.RdrfError, match="empty mesh"):
        M.write_obj(str(path), verts[:0], faces[:0], uv[:0], tex[:0])


@pytest.mark.parametrize("q", QS)
def test_the_point_bound_holds_for_a_float32_evaluation_in_the_kernels_order(q):
    """_bake_prim.points(dtype=float32) is the kernel's arithmetic, operation by operation; its distance to the float64 points
    stays inside the written bound, also where w0 cancels and v0 is the only vertex away from the origin"""
    rng = np.random.default_rng(q)
    nv, F = 12, 7
    verts = (rng.standard_normal((nv, 3)) * 2.5).astype(np.float32)
    faces = np.stack([rng.permutation(nv)[:3] for _ in range(F)]).astype(np.int32)
    verts[faces[0, 0]] = [1000.0, -777.0, 3.0]       # a far v0 with its neighbours at the origin: only the cancellation term
    verts[faces[0, 1]] = 0.0                          # of the bound is left on the edge opposite v0
    verts[faces[0, 2]] = 0.0
    Wt = 3 * q + 1
    ref = B.points(verts, faces, q, Wt)
    f32 = B.points(verts, faces, q, Wt, dtype=np.float32)
    assert f32["points"].dtype == np.float32
    err = np.abs(f32["points"].astype(np.float64) - ref["points"])
    owned = ref["face"] >= 0
    assert owned.sum() == (F // 2) * q * q + (q * (q + 1) // 2 if F & 1 else 0)
    assert (err <= ref["bound"]).all(), float((err / np.maximum(ref["bound"], 1e-300)).max())
    ratio = float((err[owned] / ref["bound"][owned]).max())
    print(f"q = {q}: worst float32 error / bound {ratio:.3f}")
    record_margin(f"bake.points.q{q} float32 evaluation", ratio)
    ok = ref["short_ok"]
    assert ok.sum() >= F and (err[ok] <= ref["short_form"][ok]).all()   # away from the cancellation: the short form, k = 8
    record_margin(f"bake.points.q{q} float32 evaluation, short form", float((err[ok] / ref["short_form"][ok]).max()))
    j, i = np.meshgrid(np.arange(q), np.arange(q), indexing="ij")
    w32, w64 = B.weights(q, i, j, i + j > q - 1, np.float32), B.weights(q, i, j, i + j > q - 1)
    exact = all(np.array_equal(a.astype(np.float64), b) for a, b in zip(w32, w64))
    assert exact == (q == 4)   # q = 4: the divisors are 2 and 1, every weight dyadic, the GPU test can ask for equal bits
    if q == 5:   # k u (|w0||v0| + |w1||v1| + |w2||v2|) alone does not bound the evaluation where w0 cancels
        assert (err > ref["issue_form"]).any()


def test_argument_errors():
    verts = torch.zeros(4, 3)
    faces = torch.tensor([[0, 1, 2], [1, 2, 3]], dtype=torch.int32)
    for q in (3, 65, 8.0, True):
        with pytest.raises(L.RdrfError, match="texels must be"):
            M.atlas_layout(2, q)
        with pytest.raises(L.RdrfError, match="texels must be"):
            M.atlas_uv(2, q)
        with pytest.raises(L.RdrfError, match="texels must be"):
            M.bake_texels(verts, faces, q)
        with pytest.raises(L.RdrfError, match="texels must be"):
            M.bake_texture(None, verts, faces, texels=q)
        with pytest.raises(L.RdrfError, match="texels must be"):
            M.export_mesh("no_such_checkpoint.th", "out.ply", texture=q)
    for width in (7, 0, -8):
        with pytest.raises(L.RdrfError, match="holds no square"):
            M.atlas_layout(2, 8, width)
        with pytest.raises(L.RdrfError, match="holds no square"):
            M.bake_texels(verts, faces, 8, width)
    assert M.atlas_layout(2, 8, 8) == (8, 8, 1)
    for bad in (torch.tensor([[0, 1, 4]], dtype=torch.int32), torch.tensor([[0, -1, 2]], dtype=torch.int32)):
        with pytest.raises(L.RdrfError, match="face indices run from"):
            M.bake_texels(verts, bad, 4)
    with pytest.raises(L.RdrfError, match="faces must be"):
        M.bake_texels(verts, faces.long(), 4)
    with pytest.raises(L.RdrfError, match="view must be"):
        M.bake_texels(verts, faces, 4, view="up")
    with pytest.raises(L.RdrfError, match="CPU tensor"):   # the arguments are right: the kernels run on the device only
        M.bake_texels(verts, faces, 4)

    import rodynrf
    from _gpu_util import COMMON
    aabb = torch.tensor([[-1.5, -1.67, -1.0], [1.5, 1.67, 1.0]])
    kw = dict(COMMON, near_far=[0.0, 1.0], density_shift=-10.0, fea2denseAct="relu")
    st = rodynrf.TensorVMSplit(aabb, [9, 11, 7], 3, "cpu", shadingMode="MLP_Fea", fea_pe=2, **kw)
    dy = rodynrf.TensorVMSplit_TimeEmbedding(aabb, [9, 11, 7], 3, "cpu", shadingMode="MLP_Fea_late_view", fea_pe=0, **kw)
    with pytest.raises(L.RdrfError, match="tensorf must be the dynamic field"):
        M.bake_texture(st, verts, faces, 0.0, static=st)      # static= next to a static field
    with pytest.raises(L.RdrfError, match="tensorf_static must be the static field"):
        M.bake_texture(dy, verts, faces, 0.0, static=dy)
    with pytest.raises(L.RdrfError, match="pass t"):
        M.bake_texture(dy, verts, faces)
    with pytest.raises(L.RdrfError, match="pass t"):
        M.bake_texture(dy, verts, faces, static=st)
    with pytest.raises(L.RdrfError, match="face indices run from"):
        M.bake_texture(st, verts, torch.tensor([[0, 1, 9]], dtype=torch.int32))
    with pytest.raises(L.RdrfError, match="chunks of"):
        M.bake_texture(st, verts, faces, texels=8, _chunk=63)
    for fill in ((0, 0), (0, 0, 256), (0, -1, 0), (1, 2, 3, 4), (0.5, 0, 0), 7):
        with pytest.raises(L.RdrfError, match="fill must be"):
            M.bake_texture(st, verts, faces, fill=fill)
    for miss in (dict(H=27.0, W=48.0), dict(focal=41.5)):
        with pytest.raises(L.RdrfError, match="needs H, W and focal"):   # before any device work
            M.textured_mesh(st, None, space="world", **miss)
    with pytest.raises(L.RdrfError, match="needs texture="):
        M.export_mesh(st, "out.ply", color_view="normal")
    with pytest.raises(L.RdrfError, match="colours come from"):
        M.export_mesh(st, "out.ply", texture=4, colors=verts)   # a PLY-only argument next to texture=


def test_native_refusals_need_no_device():
    """rdrf_bake_* check q, the width, the height, the chunk and null pointers before any device work"""
    import ctypes as C
    view = (C.c_float * 3)(0, 0, 1)
    fill = (C.c_ubyte * 3)(0, 0, 0)
    one = C.c_void_p(256)   # a pointer that is not null and never followed: every call below is refused first
    lib = L.lib
    for q, Wt, Ht, word in ((3, 16, 16, "texels per square"), (65, 128, 128, "texels per square"), (8, 7, 8, "holds no square"),
                            (8, 16, 8, "need 16 rows"), (8, 1 << 16, 1 << 15, "the limit is 2^31 - 1")):
        assert lib.rdrf_bake_texels(one, one, 6, q, Wt, Ht, view, one, one, one, None) == -1
        assert word in lib.rdrf_last_error().decode(), lib.rdrf_last_error()
        assert lib.rdrf_bake_texture(one, 0, one, one, one, 6, q, Wt, Ht, view, None, fill, 1, one, one, 1 << 30, None) == -1
        assert word in lib.rdrf_last_error().decode(), lib.rdrf_last_error()
    assert lib.rdrf_bake_texels(None, None, 2, 8, 8, 8, view, None, one, one, None) == -1
    assert "bad arguments" in lib.rdrf_last_error().decode()
    assert lib.rdrf_bake_texels(one, one, 0, 8, 8, 0, view, None, None, None, None) == 0   # an empty atlas: nothing to do
    assert lib.rdrf_bake_texture(one, 0, one, one, one, 2, 8, 8, 8, view, None, None, 1, one, one, 1 << 30, None) == -1
    assert "no fill colour" in lib.rdrf_last_error().decode()
    assert lib.rdrf_bake_ws_bytes(0, 0, 3, 1) == 0 and lib.rdrf_bake_ws_bytes(0, 0, 8, 0) == 0
    assert lib.rdrf_bake_ws_bytes(0, 0, 64, 4097) == 0 and lib.rdrf_bake_ws_bytes(0, 0, 64, 4096) > 0
    # the workspace follows the chunk: one carve, shared with the point query's and the scene's
    for scene, dyn in ((0, 0), (0, 1), (1, 1)):
        small, big = lib.rdrf_bake_ws_bytes(scene, dyn, 8, 4), lib.rdrf_bake_ws_bytes(scene, dyn, 8, 400)
        sub = max([lib.rdrf_query_points_ws_bytes(d, 8 * 8 * 4, 0) for d in ((0, 1) if scene else (dyn,))]
                  + ([lib.rdrf_scene_alpha_ws_bytes(8 * 8 * 4, 1)] if scene else []))
        up = lambda n: (n + 255) // 256 * 256
        M4 = 8 * 8 * 4
        assert small == (3 + 2 * scene) * up(M4 * 12) - scene * (up(M4 * 12) - up(M4 * 4)) + up(sub) and big > small
