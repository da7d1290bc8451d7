"""GPU tests of the texture atlases (csrc/rdrf_bake.hip; mesh.bake_texels / bake_texture / textured_mesh / export_mesh(texture=)):
the geometry stage against the float64 reference of tests/_bake_prim.py (bit for bit where the weights are dyadic, inside the
written bounds elsewhere), poisoned buffers with slack around them, the colours bit for bit against query_points (and the torch
composition of scene_vertex_colors) at the points the geometry stage returns, chunking, and the meshes and files on top.

Small hand-made meshes: nv <= 64, F <= 2R + 1, R forced to 2 or 3 through the width."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import _bake_prim as B
from _gpu_util import COMMON
from _twin import same_bits
from _util import pkg, record_margin

pytestmark = pytest.mark.gpu
DEV = "cuda"
GRID, TSIZE = [9, 11, 7], 3
AABB = torch.tensor([[-1.5, -1.67, -1.0], [1.5, 1.67, 1.0]])
AABB_S = AABB * torch.tensor([[0.9], [0.8]])
FILL = (7, 200, 33)
VIEW = (0.0, 0.6, 0.8)
T = 0.3
_cache = {}


def fields():
    """fresh fields on the suite's small grid, conditioned as tests/test_gpu_scene_volume.py conditions them: both sigmas of
    order 1 and the blending over most of (0, 1), so that the scene's owner is neither 0 nor 1; the appearance lines are
    scaled up as well, since the colours of a freshly initialised field differ by less than one 8-bit level"""
    if "fields" not in _cache:
        import rodynrf
        torch.manual_seed(11)
        kw = dict(COMMON, near_far=[0.0, 1.0], density_shift=0.0, fea2denseAct="relu")
        st = rodynrf.TensorVMSplit(AABB_S, GRID, TSIZE, DEV, shadingMode="MLP_Fea", fea_pe=2, **kw)
        dy = rodynrf.TensorVMSplit_TimeEmbedding(AABB, GRID, TSIZE, DEV, shadingMode="MLP_Fea_late_view", fea_pe=0, **kw)
        with torch.no_grad():
            for p in list(st.density_line) + list(dy.density_line) + list(dy.blending_line):
                p.mul_(6.0)
            for p in list(st.app_line) + list(dy.app_line):
                p.mul_(10.0)
            dy.density_layer2.weight.mul_(4.0)
            dy.blending_layer2.weight.mul_(12.0)
        _cache["fields"] = (st, dy)
    return _cache["fields"]


def mesh(F, nv=16, seed=0, integers=False):
    """seeded vertices inside the dynamic field's box (or small integers) and F faces of three different vertices each"""
    rng = np.random.default_rng(seed)
    if integers:
        verts = rng.integers(-8, 9, (nv, 3)).astype(np.float32)
    else:
        verts = (rng.uniform(-1, 1, (nv, 3)) * np.array([1.4, 1.5, 0.9])).astype(np.float32)
    faces = np.array([rng.permutation(nv)[:3] for _ in range(F)], dtype=np.int32).reshape(F, 3)
    return verts, faces


def dev(verts, faces):
    return torch.from_numpy(verts).to(DEV), torch.from_numpy(faces).to(DEV)


def quantise(rgb):
    return torch.round(rgb.clamp(0.0, 1.0) * 255.0).to(torch.uint8)


def with_fill(face, colours, fill=FILL):
    return torch.where((face >= 0)[..., None], colours, torch.tensor(fill, dtype=torch.uint8, device=colours.device))


# ---- 1. the geometry stage ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [2, 3])
def test_texel_points_are_the_reference_bit_for_bit_where_the_weights_are_dyadic(R):
    M = pkg("mesh")
    q, F = 4, 2 * R + 1
    width = R * q + 1
    verts, faces = mesh(F, integers=True)
    view = (0.3, -0.5, 0.8125)
    out = M.bake_texels(*dev(verts, faces), q, width, view)
    ref = B.points(verts, faces, q, width)
    Wt, Ht, _ = B.layout(F, q, width)
    assert tuple(out["points"].shape) == (Ht, Wt, 3) and out["face"].dtype == torch.int32
    face = out["face"].cpu().numpy()
    assert np.array_equal(face, ref["face"])
    assert out["points"].cpu().numpy().tobytes() == ref["points"].astype(np.float32).tobytes()
    assert (ref["bound"][face >= 0] > 0).all()
    vd = out["viewdirs"].cpu().numpy()
    assert (vd[face >= 0] == np.array(view, dtype=np.float32)).all()          # one shared view, handed on bit for bit
    assert (vd[face < 0] == np.array([0, 0, 1], dtype=np.float32)).all() and (face < 0).sum() > 0
    assert (out["points"].cpu().numpy()[face < 0] == 0).all()


@pytest.mark.parametrize("q", [5, 8])
def test_texel_points_stay_inside_the_written_bound(q):
    M = pkg("mesh")
    R = 3
    F, width = 2 * R + 1, R * q + q // 2
    verts, faces = mesh(F, nv=24, seed=q)
    verts[faces[0, 0]] = [1000.0, -777.0, 3.0]   # the cancellation of w0 on the edge opposite a far v0 (tests/_bake_prim.py)
    verts[faces[0, 1]] = 0.0
    verts[faces[0, 2]] = 0.0
    out = M.bake_texels(*dev(verts, faces), q, width)
    ref = B.points(verts, faces, q, width)
    assert np.array_equal(out["face"].cpu().numpy(), ref["face"])
    got = out["points"].cpu().numpy()
    err = np.abs(got.astype(np.float64) - ref["points"])
    owned = ref["face"] >= 0
    ratio = float((err[owned] / ref["bound"][owned]).max())
    print(f"q = {q}: texel point error / bound {ratio:.3f}")
    record_margin(f"bake.points.q{q}", ratio)
    assert (err <= ref["bound"]).all(), ratio
    ok = ref["short_ok"]
    short = float((err[ok] / ref["short_form"][ok]).max())
    record_margin(f"bake.points.q{q} short form", short)
    assert ok.sum() >= F and short <= 1.0   # away from the cancellation: k u (|w0||v0| + |w1||v1| + |w2||v2|) with k = 8
    # the kernel's arithmetic is the float32 evaluation of the reference, operation by operation
    assert got.tobytes() == B.points(verts, faces, q, width, dtype=np.float32)["points"].tobytes()


def test_normal_view_directions():
    M = pkg("mesh")
    q, R = 5, 3
    F, width = 2 * R + 1, R * q + 2
    verts, faces = mesh(F, nv=23, seed=3)
    faces[2] = [faces[2, 0], faces[2, 1], faces[2, 1]]          # a zero-area face
    nan_vertex = 23
    verts = np.concatenate((verts, np.array([[np.nan, 0.25, 0.5]], dtype=np.float32)))
    faces[5] = [1, nan_vertex, 2]                                 # a face with a NaN vertex
    tv, tf = dev(verts, faces)
    out = M.bake_texels(tv, tf, q, width, view="normal")
    face = out["face"].cpu().numpy()
    vd = out["viewdirs"].cpu().numpy()
    d, bound, ok = B.face_dirs(verts, faces)
    assert list(np.nonzero(~ok)[0]) == [2, 5]
    worst = 0.0
    for f in range(F):
        mine = vd[face == f]
        assert len(mine) > 0 and (mine == mine[0]).all()          # one direction per face, gutter texels included
        if not ok[f]:
            assert (mine[0] == np.array([0, 0, 1], dtype=np.float32)).all()
            continue
        err = np.abs(mine[0].astype(np.float64) - d[f])
        worst = max(worst, float((err / bound[f]).max()))
        assert (err <= bound[f]).all(), (f, err, bound[f])
        # opposite to the normal that face_vertex_normals gives the face on its own
        n = M.face_vertex_normals(tv, tf[f:f + 1])[int(faces[f, 0])].cpu().numpy().astype(np.float64)
        assert abs(float(n @ n) - 1.0) < 1e-5 and float(n @ mine[0].astype(np.float64)) < -1.0 + 1e-5
    print(f"view = normal: direction error / bound {worst:.3f}")
    record_margin("bake.normal", worst)
    assert (vd[face < 0] == np.array([0, 0, 1], dtype=np.float32)).all()


# ---- 2. poisoned buffers ----------------------------------------------------------------------------------------------------------
SLACK = 96


def padded(n, dtype, byte, slack=SLACK):
    """a buffer of n elements with `slack` elements of poison on each side, all bytes `byte`"""
    full = torch.full(((n + 2 * slack) * torch.empty(0, dtype=dtype).element_size(),), byte, dtype=torch.uint8, device=DEV).view(dtype)
    return full, full[slack:slack + n]


def slack_is(full, n, byte, slack=SLACK):
    raw = full.view(torch.uint8)
    e = full.element_size()
    return bool((raw[:slack * e] == byte).all()) and bool((raw[(slack + n) * e:] == byte).all())


@pytest.mark.parametrize("F,Ht_extra", [(0, 1), (5, 0), (7, 0), (7, 1)], ids=["empty", "odd", "last_row_partly_used", "taller_atlas"])
@pytest.mark.parametrize("which", ["static", "dynamic", "scene"])
def test_poisoned_buffers(which, F, Ht_extra):
    """every byte of the atlas, the points and the directions is written whatever was there, texels without a face are `fill`
    / 0 / (0, 0, 1) / -1 exactly, and the slack around each buffer is untouched.  R = 3: F = 7 leaves the last row with one
    square of three and its upper half without a face"""
    L, P = pkg(), pkg("_params")
    st, dy = fields()
    field = st if which == "static" else dy
    q, R = 4, 3
    Wt = R * q + 3
    verts, faces = mesh(F, seed=F)
    Ht = B.layout(F, q, Wt)[1] + Ht_extra * q
    n = Wt * Ht
    tv, tf = dev(verts, faces)
    own = B.ownership(F, q, Wt, Ht)["face"]
    view = (C.c_float * 3)(*VIEW)
    fill = (C.c_ubyte * 3)(*FILL)
    stream = L.stream_of(tv)
    results = []
    for byte in (0xA5, 0xFF):   # 0xFF: every float a NaN
        pf, p = padded(n * 3, torch.float32, byte)
        vf, v = padded(n * 3, torch.float32, byte)
        ff, f = padded(n, torch.int32, byte)
        xf, x = padded(n * 3, torch.uint8, byte)
        L.check(L.lib.rdrf_bake_texels(L.ptr(tv), L.ptr(tf), F, q, Wt, Ht, view, L.ptr(p), L.ptr(v), L.ptr(f), stream), "rdrf_bake_texels")
        squares = 2
        t_dev = torch.full((1,), T, device=DEV)
        ws_bytes = L.lib.rdrf_bake_ws_bytes(int(which == "scene"), int(field.DYNAMIC), q, squares)
        wf, ws = padded(ws_bytes, torch.uint8, byte, 256)   # the scratch keeps its 256-byte alignment
        Pf, cfg = P.field_structs(field, field._param_list(), "ndc")
        common = (L.ptr(tv), L.ptr(tf), F, q, Wt, Ht, view, L.ptr(t_dev))
        tail = (fill, squares, L.ptr(x), L.ptr(ws), ws_bytes, stream)
        if which == "scene":
            Ps, cs = P.field_structs(st, st._param_list(), "ndc")
            L.check(L.lib.rdrf_bake_scene_texture(C.byref(Ps), C.byref(cs), C.byref(Pf), C.byref(cfg), *common, float(dy._step_host),
                                                  None, None, *tail), "rdrf_bake_scene_texture")
        else:
            L.check(L.lib.rdrf_bake_texture(C.byref(Pf), int(field.DYNAMIC), C.byref(cfg), *common, *tail), "rdrf_bake_texture")
        torch.cuda.synchronize()
        assert slack_is(pf, n * 3, byte) and slack_is(vf, n * 3, byte) and slack_is(ff, n, byte) and slack_is(xf, n * 3, byte)
        assert slack_is(wf, ws_bytes, byte, 256)
        face = f.view(Ht, Wt).cpu().numpy()
        assert np.array_equal(face, own)
        pts, vds, tex = p.view(Ht, Wt, 3).cpu().numpy(), v.view(Ht, Wt, 3).cpu().numpy(), x.view(Ht, Wt, 3).cpu().numpy()
        assert np.isfinite(pts).all() and np.isfinite(vds).all()
        assert (pts[face < 0] == 0).all() and (vds[face < 0] == np.array([0, 0, 1], dtype=np.float32)).all()
        assert (tex[face < 0] == np.array(FILL, dtype=np.uint8)).all()
        results.append((pts, vds, tex))
    for a, b in zip(*results):   # nothing of the poison shows through: every byte was written
        assert a.tobytes() == b.tobytes()
    assert (own < 0).sum() >= 3 * Ht and ((own >= 0).sum() > 0) == (F > 0)
    if F > 0:
        tex = results[0][2]
        assert len(np.unique(tex[own >= 0].reshape(-1, 3), axis=0)) > 1   # the owned texels carry the field's colours


# ---- 3. colours -------------------------------------------------------------------------------------------------------------------
def colour_case(q=5, R=3, F=14, seed=2):
    """seven squares in rows of three: chunks of two squares split the batch into four, with edges inside the atlas rows"""
    verts, faces = mesh(F, nv=20, seed=seed)
    return dev(verts, faces) + (q, R * q + 1)


@pytest.mark.parametrize("view", [VIEW, "normal"], ids=["shared_view", "normal"])
@pytest.mark.parametrize("which", ["static", "dynamic"])
def test_baked_colours_are_the_point_query_bit_for_bit(which, view):
    M = pkg("mesh")
    st, dy = fields()
    field, t = (st, None) if which == "static" else (dy, T)
    tv, tf, q, width = colour_case()
    geo = M.bake_texels(tv, tf, q, width, view)
    tex, uv = M.bake_texture(field, tv, tf, t, q, width, view, FILL)
    rgb = field.query_points(geo["points"], t, geo["viewdirs"], want=("rgb",))["rgb"]
    want = with_fill(geo["face"], quantise(rgb))
    assert tex.dtype == torch.uint8 and tex.shape == want.shape and torch.equal(tex, want)
    owned = tex[geo["face"] >= 0]
    assert len(torch.unique(owned.view(-1, 3), dim=0)) > 1
    assert np.array_equal(uv.cpu().numpy(), B.uv(tf.shape[0], q, width).astype(np.float32)) and uv.device == tv.device
    # chunks of two squares: four chunks for the seven squares, their edges inside the atlas rows of three
    assert torch.equal(M.bake_texture(field, tv, tf, t, q, width, view, FILL, _chunk=2 * q * q + 3)[0], tex)
    assert torch.equal(M.bake_texture(field, tv, tf, t, q, width, view, FILL, _chunk=q * q)[0], tex)
    if view != "normal":   # the view is read
        assert not torch.equal(M.bake_texture(field, tv, tf, t, q, width, (0.0, 0.0, 1.0), FILL)[0], tex)
    if which == "dynamic":
        assert not torch.equal(M.bake_texture(field, tv, tf, -0.7, q, width, view, FILL)[0], tex)   # and the time


@pytest.mark.parametrize("view", [VIEW, "normal"], ids=["shared_view", "normal"])
def test_scene_bake_is_the_composition_of_scene_vertex_colors_bit_for_bit(view):
    M, A = pkg("mesh"), pkg("alpha")
    st, dy = fields()
    tv, tf, q, width = colour_case(seed=5)
    geo = M.bake_texels(tv, tf, q, width, view)
    tex, _ = M.bake_texture(dy, tv, tf, T, q, width, view, FILL, static=st)
    pts, vd = geo["points"].reshape(-1, 3), geo["viewdirs"].reshape(-1, 3)
    o = A.scene_alpha_volume(st, dy, pts, [T], want=("owner",))["owner"]
    rgb_d = dy.query_points(pts, T, vd, want=("rgb",))["rgb"]
    rgb_s = st.query_points(pts, None, vd, want=("rgb",))["rgb"]
    rgb = o * rgb_d + (1.0 - o) * rgb_s                      # the expression of mesh.scene_vertex_colors
    want = with_fill(geo["face"], quantise(rgb).view(tex.shape))
    assert torch.equal(tex, want)
    oo = o.view(geo["face"].shape)[geo["face"] >= 0]
    print(f"owner at the owned texels: mean {float(oo.mean()):.3f}, {float(oo.min()):.3f} .. {float(oo.max()):.3f}")
    assert not torch.equal(tex, M.bake_texture(dy, tv, tf, T, q, width, view, FILL)[0])   # the static field shows
    if view != "normal":   # at a vertex (a corner texel of a lower face) the texel is the colour scene_vertex_colors gives it
        col = M.scene_vertex_colors(st, dy, tv, T, view)
        f = 4
        s = f >> 1
        y, x = (s // 3) * q, (s % 3) * q
        assert int(geo["face"][y, x]) == f and torch.equal(tex[y, x], col[int(tf[f, 0])])
    assert torch.equal(M.bake_texture(dy, tv, tf, T, q, width, view, FILL, static=st, _chunk=2 * q * q)[0], tex)
    assert torch.equal(M.bake_texture(dy, tv, tf, T, q, width, view, FILL, static=st, _chunk=3 * q * q - 1)[0], tex)


@pytest.mark.parametrize("masked", ["both", "static", "dynamic"])
def test_scene_bake_reads_each_fields_alpha_mask(masked):
    """the bake hands each field's alphaMask to the scene's owner, as scene_vertex_colors does: masks of different grids, on
    one field or on both, against the torch composition and against the bake without masks.  A mask sample is trilinear, so
    the masks are sparse (a tenth of the cells set, as in tests/test_gpu_scene_volume.py): most points lie in empty cells"""
    import rodynrf
    M, A = pkg("mesh"), pkg("alpha")
    st, dy = fields()
    tv, tf, q, width = colour_case(seed=5)
    g = torch.Generator().manual_seed(5)
    m_s = rodynrf.AlphaGridMask(DEV, AABB_S, (torch.rand(7, 11, 9, TSIZE, generator=g) < 0.1).float(), TSIZE)
    m_d = rodynrf.AlphaGridMask(DEV, AABB, (torch.rand(5, 6, 4, TSIZE, generator=g) < 0.12).float(), TSIZE)
    free, _ = M.bake_texture(dy, tv, tf, T, q, width, VIEW, FILL, static=st)
    geo = M.bake_texels(tv, tf, q, width, VIEW)
    pts, vd = geo["points"].reshape(-1, 3), geo["viewdirs"].reshape(-1, 3)
    assert st.alphaMask is None and dy.alphaMask is None
    st.alphaMask = m_s if masked in ("both", "static") else None
    dy.alphaMask = m_d if masked in ("both", "dynamic") else None
    try:
        tex, _ = M.bake_texture(dy, tv, tf, T, q, width, VIEW, FILL, static=st, _chunk=2 * q * q)
        o = A.scene_alpha_volume(st, dy, pts, [T], want=("owner",))["owner"]   # masks="fields"
    finally:
        st.alphaMask, dy.alphaMask = None, None
    rgb = o * dy.query_points(pts, T, vd, want=("rgb",))["rgb"] + (1.0 - o) * st.query_points(pts, None, vd, want=("rgb",))["rgb"]
    assert torch.equal(tex, with_fill(geo["face"], quantise(rgb).view(tex.shape)))
    assert not torch.equal(tex, free)


def test_a_faces_texels_do_not_depend_on_the_other_faces():
    M = pkg("mesh")
    st, dy = fields()
    tv, tf, q, width = colour_case()
    full, _ = M.bake_texture(dy, tv, tf, T, q, width, "normal", FILL, static=st)
    part, _ = M.bake_texture(dy, tv, tf[2:4].contiguous(), T, q, width, "normal", FILL, static=st)   # square 1 becomes square 0
    assert torch.equal(part[:q, :q], full[:q, q:2 * q]) and part.shape[0] == q
    shuffled = tf.clone()
    shuffled[[0, 1, 8, 9]] = tf[[8, 9, 0, 1]]                                                        # squares 0 and 4 swap
    swapped, _ = M.bake_texture(dy, tv, shuffled, T, q, width, "normal", FILL, static=st)
    assert torch.equal(swapped[:q, :q], full[q:2 * q, q:2 * q]) and torch.equal(swapped[q:2 * q, q:2 * q], full[:q, :q])
    assert torch.equal(swapped[:q, q:], full[:q, q:])


# ---- 4. meshes and files --------------------------------------------------------------------------------------------------------
LATTICE = (12, 10, 9)


def _level(alpha):
    """the median of the samples above the volume's minimum (a relu field is 0 over much of its box): about half of them
    inside, whatever the distribution"""
    v = alpha.flatten()
    v = v[v > v.min()]
    return float(v.kthvalue(max(1, v.numel() // 2)).values)


@pytest.mark.parametrize("scene", [False, True], ids=["field", "scene"])
def test_textured_mesh_and_export(scene, tmp_path):
    import rodynrf
    st, dy = fields()
    static = st if scene else None
    if scene:
        level = _level(rodynrf.scene_dense_alpha(st, dy, LATTICE, times=[T])[0])
        verts, faces, nrm = rodynrf.scene_mesh(st, dy, T, level, LATTICE, normals=True, simplify=2)
    else:
        level = _level(dy.getDenseAlpha(LATTICE, times=[T])[0])
        verts, faces, nrm = rodynrf.field_mesh(dy, T, level, LATTICE, normals=True, simplify=2)
    assert verts.shape[0] > 0 and faces.shape[0] > 0
    q = 4
    tex, uv = rodynrf.bake_texture(dy, verts, faces, T, q, view=VIEW, static=static)       # simplify -> bake, by hand
    out = rodynrf.textured_mesh(dy, T, level, LATTICE, q, VIEW, normals=True, simplify=2, static=static)
    assert len(out) == 5
    for a, b in zip(out, (verts, faces, nrm, uv, tex)):
        assert same_bits(a, b)
    assert (tex.shape[1], tex.shape[0]) == rodynrf.atlas_layout(faces.shape[0], q)[:2] and int(tex.max()) > int(tex.min())
    four = rodynrf.textured_mesh(dy, T, level, LATTICE, q, VIEW, simplify=2, static=static)
    assert len(four) == 4 and same_bits(four[2], uv) and same_bits(four[3], tex)
    dense = rodynrf.textured_mesh(dy, T, level, LATTICE, q, VIEW, static=static)               # the texture follows the mesh
    assert dense[1].shape[0] > faces.shape[0] and (dense[3].shape[1], dense[3].shape[0]) == rodynrf.atlas_layout(dense[1].shape[0], q)[:2]
    # world space moves the vertices and keeps uv and texels
    H, W, focal = 27.0, 48.0, 41.5
    world = rodynrf.textured_mesh(dy, T, level, LATTICE, q, VIEW, space="world", H=H, W=W, focal=focal, simplify=2, static=static)
    assert same_bits(world[0], pkg("mesh").ndc_to_world(verts, H, W, focal)) and not torch.equal(world[0], verts)
    assert same_bits(world[1], faces) and same_bits(world[2], uv) and same_bits(world[3], tex)
    # the three files, and what read_obj makes of them
    path = str(tmp_path / "mesh.ply")
    ret = rodynrf.export_mesh(dy, path, T, level, gridSize=LATTICE, texture=q, color_view=VIEW, normals=True, simplify=2, static=static)
    for a, b in zip(ret, out):
        assert same_bits(a, b)
    assert sorted(os.listdir(tmp_path)) == ["mesh.mtl", "mesh.obj", "mesh.png"]
    back = rodynrf.read_obj(str(tmp_path / "mesh.obj"))
    for key, o in zip(("verts", "faces", "normals", "uv", "texture"), out):
        assert back[key].tobytes() == o.cpu().numpy().tobytes(), key
    ret = dy.export_mesh(str(tmp_path / "n.obj"), T, level, gridSize=LATTICE, texture=q, color_view="normal", simplify=2, static=static)
    want = rodynrf.bake_texture(dy, verts, faces, T, q, view="normal", static=static)[0]
    assert len(ret) == 4 and same_bits(ret[3], want) and not torch.equal(want, tex)
    assert np.array_equal(rodynrf.read_obj(str(tmp_path / "n.obj"))["texture"], want.cpu().numpy())
