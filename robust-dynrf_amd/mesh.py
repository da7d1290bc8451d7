"""Isosurface meshes of dense alpha volumes (the reference's --export_mesh, train.py:107-118 -> utils.py:188-247
convert_sdf_samples_to_ply) on the kernels of csrc/rdrf_iso.hip: marching tetrahedra on the device, an indexed mesh in a
fixed order, PLY through numpy.

Where this departs from the reference on purpose: the lattice positions are the dense_xyz points getDenseAlpha sampled
(spacing extent / (G - 1); the reference's voxel_size = extent / G is off by G / (G - 1)), and triangles are
counter-clockwise seen from the low-value side (the reference reverses skimage's faces; pass flip=True for the other
winding).  DESIGN.md, "Isosurface meshes", has the algorithm and the ordering rules.
"""
import ctypes as C
import math
import os
import struct
import zlib

import numpy as np
import torch

from . import _lib as L

CAP_VALUE = -1.0e30   # "minus infinity" of cap=True: finite, so t = (level - v_lo) / (v_hi - v_lo) rounds to exactly 1


def _aabb6(aabb):
    a = torch.as_tensor(aabb, dtype=torch.float32).detach().cpu().reshape(-1)
    if a.numel() != 6:
        raise L.RdrfError(f"aabb must hold min xyz and max xyz, not {a.numel()} values")
    return a


def _cap(volume, aabb):
    """a [G0,G1,G2] volume with one sample of CAP_VALUE around it, the aabb grown by one cell per side"""
    G = volume.shape
    padded = volume.new_full((G[0] + 2, G[1] + 2, G[2] + 2), CAP_VALUE)
    padded[1:-1, 1:-1, 1:-1] = volume
    a = aabb.double().view(2, 3)
    cell = (a[1] - a[0]) / torch.tensor([g - 1 for g in G], dtype=torch.float64)
    return padded, torch.stack((a[0] - cell, a[1] + cell)).float().reshape(-1)


@torch.no_grad()
def extract_isosurface(volume, level, aabb, t_index=0, normals=False, flip=False, cap=False, simplify=None):
    """volume: device tensor [G0,G1,G2] or [G0,G1,G2,T] (slice t_index is meshed, in place) -> (verts [nv,3] float32,
    faces [nf,3] int32[, normals [nv,3]]).  A sample is inside iff v >= level; verts ascend in (lattice point, edge kind),
    faces in (cube, tetrahedron, triangle).  cap=True closes the surface where it reaches the volume boundary.
    One host read (the two counts) between the counting and the emitting launches; an empty mesh skips the second.
    simplify=K: the mesh is then clustered (simplify_mesh) on the lattice simplify_lattice(aabb, volume.shape, K, cap)."""
    L.require_device(volume)
    if volume.dim() not in (3, 4):
        raise L.RdrfError(f"extract_isosurface: the volume must be [G0,G1,G2] or [G0,G1,G2,T], not {tuple(volume.shape)}")
    vol = L.f32c(volume)
    T = 1 if vol.dim() == 3 else int(vol.shape[3])
    t_index = int(t_index)
    if not 0 <= t_index < T:
        raise L.RdrfError(f"extract_isosurface: t_index {t_index} of {T} slices")
    box = _aabb6(aabb)
    if cap:   # only the slice that is meshed is copied
        vol, box = _cap(vol if vol.dim() == 3 else vol[..., t_index], box)
        T, t_index = 1, 0
    G0, G1, G2 = (int(v) for v in vol.shape[:3])
    dev, stream = vol.device, L.stream_of(vol)
    nbytes = L.lib.rdrf_iso_ws_bytes(G0, G1, G2)
    ws = L.workspace(dev, nbytes) if nbytes else None   # 0: a refused shape, which rdrf_iso_count reports by name
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    L.check(L.lib.rdrf_iso_count(L.ptr(vol), G0, G1, G2, T, t_index, float(level), L.ptr(ws), 0 if ws is None else ws.numel(),
                                 L.ptr(counts), stream), "rdrf_iso_count")
    nv, nf = (int(v) for v in counts.cpu().tolist())   # the one sync
    verts = torch.empty(nv, 3, dtype=torch.float32, device=dev)
    faces = torch.empty(nf, 3, dtype=torch.int32, device=dev)
    nrm = torch.empty(nv, 3, dtype=torch.float32, device=dev) if normals else None
    if nv > 0:
        box_c = (C.c_float * 6)(*[float(v) for v in box])
        L.check(L.lib.rdrf_iso_emit(L.ptr(vol), G0, G1, G2, T, t_index, float(level), box_c, int(bool(flip)), L.ptr(ws),
                                    L.ptr(verts), L.ptr(nrm), L.ptr(faces), nv, nf, stream), "rdrf_iso_emit")
    if simplify is not None:
        return _simplify(verts, faces, simplify_lattice(box, (G0, G1, G2), simplify), nrm, None, True, False, "extract_isosurface")
    return (verts, faces, nrm) if normals else (verts, faces)


# ---- mesh simplification: vertex clustering on the kernels of csrc/rdrf_simplify.hip -----------------------------------------
def simplify_lattice(aabb, shape, K, cap=False):
    """the clustering lattice of simplify=K for a meshed volume of `shape` = (G0, G1, G2) samples over aabb (cap=True: the
    volume and the box that cap=True meshes, one sample and one cell larger on every side): clusters K lattice cells wide from
    aabb_min, cell_a = K spacing_a, n_a = ceil((G_a - 1) / K).  Returns dict(aabb, cell, grid), the arguments of simplify_mesh."""
    if isinstance(K, bool) or not isinstance(K, int) or K < 1:
        raise L.RdrfError(f"simplify must be a whole number of lattice cells >= 1, not {K!r}")
    box = _aabb6(aabb)
    G = [int(g) for g in shape[:3]]
    if cap:
        a = box.double().view(2, 3)
        h = (a[1] - a[0]) / torch.tensor([g - 1 for g in G], dtype=torch.float64)
        box = torch.stack((a[0] - h, a[1] + h)).float().reshape(-1)
        G = [g + 2 for g in G]
    a = box.double().view(2, 3)
    cell = [float(K * (a[1, d] - a[0, d]) / (G[d] - 1)) for d in range(3)]
    return {"aabb": box, "cell": cell, "grid": [-(-(G[d] - 1) // K) for d in range(3)]}


def _simplify(verts, faces, lattice, normals, colors, drop_unreferenced, return_remap, who):
    """the two native calls on a resolved lattice dict(aabb, cell, grid) -> (verts, faces[, normals][, colors][, remap])"""
    V, F = int(verts.shape[0]), int(faces.shape[0])
    dev, stream = verts.device, L.stream_of(verts)
    origin = (C.c_float * 3)(*[float(v) for v in lattice["aabb"][:3]])
    cell = (C.c_float * 3)(*[float(v) for v in lattice["cell"]])
    n = (C.c_int * 3)(*[int(v) for v in lattice["grid"]])
    nbytes = L.lib.rdrf_simplify_ws_bytes(V, F, n)
    ws = L.workspace(dev, nbytes) if nbytes else None   # 0: a refused shape, which rdrf_simplify_count reports by name
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    remap = torch.full((V,), -1, dtype=torch.int32, device=dev) if return_remap else None
    L.check(L.lib.rdrf_simplify_count(L.ptr(verts), V, L.ptr(faces), F, origin, cell, n, int(bool(drop_unreferenced)), L.ptr(ws),
                                      0 if ws is None else ws.numel(), L.ptr(counts), L.ptr(remap), stream), f"{who}: rdrf_simplify_count")
    nv, nf = (int(v) for v in counts.cpu().tolist())   # the one sync
    out_v = torch.empty(nv, 3, dtype=torch.float32, device=dev)
    out_f = torch.empty(nf, 3, dtype=torch.int32, device=dev)
    out_n = torch.empty(nv, 3, dtype=torch.float32, device=dev) if normals is not None else None
    out_c = torch.empty(nv, 3, dtype=torch.uint8, device=dev) if colors is not None else None
    if nv > 0 or nf > 0:
        L.check(L.lib.rdrf_simplify_emit(L.ptr(verts), L.ptr(normals), L.ptr(colors), V, L.ptr(faces), F, L.ptr(ws), L.ptr(out_v),
                                         L.ptr(out_n), L.ptr(out_c), L.ptr(out_f), nv, nf, stream), f"{who}: rdrf_simplify_emit")
    out = [out_v, out_f] + [o for o in (out_n, out_c, remap) if o is not None]
    return tuple(out)


@torch.no_grad()
def simplify_mesh(verts, faces, cell=None, grid=None, aabb=None, normals=None, colors=None, drop_unreferenced=True,
                  return_remap=False):
    """Vertex clustering of a device mesh: verts [V,3] float32, faces [F,3] int32 -> (verts, faces[, normals][, colors][, remap]).
    The lattice starts at aabb_min (aabb=None: the box of the vertices, one host read): `cell` (a scalar or three numbers) gives
    n = ceil(extent / cell) cells per axis, `grid` (three counts) gives cell = extent / grid; both together are used as they
    are (what simplify_lattice returns).  A cluster's vertex is the mean of its members, its normal the normalised sum, its
    colour ([V,3] uint8) the mean rounded half up; a face survives iff its three vertices land in different clusters, in its
    old place in the order and with its winding; duplicate faces are not merged.  drop_unreferenced=False keeps the clusters
    no surviving face uses.  remap [V] int32: the new index of every old vertex, -1 where its cluster was dropped."""
    who = "simplify_mesh"
    L.require_device(verts, faces, normals, colors)
    if verts.dim() != 2 or verts.shape[1] != 3 or verts.dtype != torch.float32:
        raise L.RdrfError(f"{who}: verts must be [V,3] float32, not {tuple(verts.shape)} {verts.dtype}")
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype != torch.int32:
        raise L.RdrfError(f"{who}: faces must be [F,3] int32, not {tuple(faces.shape)} {faces.dtype}")
    if normals is not None and (normals.shape != verts.shape or normals.dtype != torch.float32):
        raise L.RdrfError(f"{who}: normals must be [V,3] float32 like verts, not {tuple(normals.shape)} {normals.dtype}")
    if colors is not None and (colors.shape != verts.shape or colors.dtype != torch.uint8):
        raise L.RdrfError(f"{who}: colors must be [V,3] uint8, not {tuple(colors.shape)} {colors.dtype}")
    if cell is None and grid is None:
        raise L.RdrfError(f"{who}: give cell (the cluster size) or grid (the cell counts over the aabb)")
    verts, faces = verts.contiguous(), faces.contiguous()
    normals = None if normals is None else normals.contiguous()
    colors = None if colors is None else colors.contiguous()
    if aabb is None:
        if verts.shape[0] == 0:
            box = torch.tensor([0.0, 0.0, 0.0, 1.0, 1.0, 1.0])
        else:
            box = torch.cat((verts.amin(0), verts.amax(0))).cpu()
    else:
        box = _aabb6(aabb)
    ext = (box[3:].double() - box[:3].double()).tolist()
    if cell is not None:
        cell = [float(v) for v in torch.as_tensor(cell, dtype=torch.float64).reshape(-1).tolist()]
        if len(cell) not in (1, 3):
            raise L.RdrfError(f"{who}: cell must be a scalar or three numbers, not {len(cell)}")
        cell = cell * 3 if len(cell) == 1 else cell
    if grid is not None:
        grid = [int(v) for v in grid]
        if len(grid) != 3:
            raise L.RdrfError(f"{who}: grid must be three counts, not {len(grid)}")
    if cell is None:
        cell = [ext[d] / grid[d] if grid[d] > 0 else 0.0 for d in range(3)]
    elif grid is None:
        if not all(c > 0.0 and c == c and c != float("inf") for c in cell):
            raise L.RdrfError(f"{who}: cell sizes must be positive and finite, not {cell}")
        if not all(e == e and abs(e) != float("inf") for e in ext):
            raise L.RdrfError(f"{who}: the box of the vertices is not finite ({box.tolist()}): pass aabb")
        grid = [max(1, int(-(-ext[d] // cell[d]))) for d in range(3)]
        if grid[0] * grid[1] * grid[2] >= 2 ** 31:
            raise L.RdrfError(f"{who}: cell {cell} over the extent {ext} gives {grid[0]} x {grid[1]} x {grid[2]} cells, the keys are below 2^31")
    return _simplify(verts, faces, {"aabb": box, "cell": cell, "grid": grid}, normals, colors, drop_unreferenced, return_remap, who)


def ndc_to_world(pts, H, W, focal):
    """the reference's NDC2world (renderer.py:1266-1274)"""
    pts_z = 2 / (torch.clamp(pts[..., 2:], min=-1.0, max=1 - 1e-6) - 1)
    pts_x = -pts[..., 0:1] * pts_z * W / 2 / focal
    pts_y = -pts[..., 1:2] * pts_z * H / 2 / focal
    return torch.cat([pts_x, pts_y, pts_z], -1)


def contract_to_world(pts):
    """the inverse of the samplers' L-inf contraction (the reference's contract2world): a point of norm n > 1 goes back to
    p / n / (2 - n); the clamp keeps the shell's outer face finite"""
    n = pts.abs().amax(-1, keepdim=True)
    return torch.where(n > 1.0, pts / n * (-1.0 / (n.clamp(max=2.0 - 1e-6) - 2.0)), pts)


@torch.no_grad()
def point_cloud(tensorf_static, tensorf, c2w, focal, H, W, t, tau=0.5, space="field", min_owner=None, max_owner=None,
                N_samples=-1, ray_type="ndc"):
    """The coloured point cloud one camera sees at time t: the surface hits (renderer.hit_view) of its H x W rays at the
    opacity level `tau`, one point per ray that hits.  Returns (xyz [M,3], rgb [M,3] in [0,1], owner [M]); the colours are
    the `rgb` map of the same call, owner is the dynamic field's share of the hit sample.  min_owner / max_owner keep the
    points with owner >= / <= the bound (0.5 and None: the moving surfaces; None and 0.5: the static scene).
    space "field": the fields' coordinates (ndc or contracted); "world": through ndc_to_world / contract_to_world."""
    from .renderer import hit_view
    if space not in ("field", "world"):
        raise L.RdrfError(f"space must be \"field\" or \"world\", not {space!r}")
    if not isinstance(tau, (int, float)):
        raise ValueError("point_cloud: one opacity level per cloud")
    h = hit_view(tensorf_static, tensorf, c2w, focal, H, W, t, float(tau), N_samples, ray_type, maps=("rgb",))
    keep = h["hit"].reshape(-1)
    owner = h["owner"].reshape(-1)
    if min_owner is not None:
        keep = keep & (owner >= float(min_owner))
    if max_owner is not None:
        keep = keep & (owner <= float(max_owner))
    xyz = h["xyz"].reshape(-1, 3)[keep]
    if space == "world":
        f = focal.to(xyz.device) if torch.is_tensor(focal) else focal
        xyz = ndc_to_world(xyz, H, W, f) if ray_type == "ndc" else contract_to_world(xyz)
    return xyz, h["rgb"].reshape(-1, 3)[keep].clamp(0.0, 1.0), owner[keep]


def face_vertex_normals(verts, faces):
    """area-weighted vertex normals from the faces (a vertex without a non-degenerate face keeps a zero normal)"""
    f = faces.long()
    a, b, c = verts[f[:, 0]], verts[f[:, 1]], verts[f[:, 2]]
    fn = torch.cross(b - a, c - a, dim=-1)
    n = torch.zeros_like(verts)
    for col in range(3):
        n.index_add_(0, f[:, col], fn)
    length = n.norm(dim=-1, keepdim=True)
    return torch.where(length > 0, n / length.clamp_min(1e-30), n)


def _to_world(field, verts, faces, space, H, W, focal):
    if space == "field":
        return verts, None
    if space != "world":
        raise L.RdrfError(f"space must be \"field\" or \"world\", not {space!r}")
    if H is None or W is None or focal is None:
        raise L.RdrfError("space=\"world\" maps NDC vertices through NDC2world and needs H, W and focal")
    world = ndc_to_world(verts, H, W, focal)
    return world, face_vertex_normals(world, faces)


def _mesh_of_slice(field, alpha, k, level, space, H, W, focal, kw, color=None):
    """color (colored_mesh): field-space vertices -> [nv,3] uint8, taken on the unsimplified mesh; clustering (simplify=K)
    comes after it and before the mapping to world space"""
    want_normals = bool(kw.get("normals", False))
    kw = dict(kw)
    K = kw.pop("simplify", None)
    out = extract_isosurface(alpha, level, field.aabb, t_index=k, **kw)
    verts, faces, nrm = out[0], out[1], (out[2] if want_normals else None)
    colors = None if color is None else color(verts)
    if K is not None:
        lattice = simplify_lattice(field.aabb, alpha.shape, K, bool(kw.get("cap", False)))
        out = _simplify(verts, faces, lattice, nrm, colors, True, False, "field_mesh")
        verts, faces = out[0], out[1]
        nrm = out[2] if want_normals else None
        colors = None if color is None else out[-1]
    world, wn = _to_world(field, verts, faces, space, H, W, focal)
    mesh = (world, faces) if not want_normals else (world, faces, (nrm if wn is None else wn))
    return mesh if color is None else mesh + (colors,)


def _check_kw(kw):
    if "colors" in kw:
        raise L.RdrfError("field_mesh / mesh_sequence take no colors=: colours come from colored_mesh, vertex_colors and "
                          "export_mesh(..., color_view=) (write_ply takes colours a caller computed)")
    bad = set(kw) - {"normals", "flip", "cap", "simplify"}
    if bad:
        raise TypeError(f"unexpected arguments {sorted(bad)}")
    K = kw.get("simplify")
    if K is not None and (isinstance(K, bool) or not isinstance(K, int) or K < 1):
        raise L.RdrfError(f"simplify must be a whole number of lattice cells >= 1, not {K!r}")


@torch.no_grad()
def field_mesh(field, t=None, level=0.005, gridSize=None, space="field", H=None, W=None, focal=None, **kw):
    """getDenseAlpha(gridSize, times=[t]) -> extract_isosurface.  t=None only for the static field (its alpha does not
    depend on the time).  space="world": the vertices of an ndc field through NDC2world (needs H, W, focal); normals are then
    recomputed from the transformed faces.  kw: normals, flip, cap, simplify (K: vertex clustering K lattice cells wide, in
    field space)."""
    _check_kw(kw)
    if t is None:
        if field.DYNAMIC:
            raise L.RdrfError("field_mesh: the dynamic field's alpha depends on the time: pass t")
        t = 0.0
    alpha, _ = field.getDenseAlpha(gridSize, times=[float(t)])
    return _mesh_of_slice(field, alpha, 0, level, space, H, W, focal, kw)


def mesh_sequence(field, times, level=0.005, gridSize=None, space="field", H=None, W=None, focal=None, **kw):
    """an iterator of one mesh per time: a single getDenseAlpha over all times, then one extraction per slice of the
    [G0,G1,G2,T] volume.  The arguments are checked here, at the call, not at the first next()."""
    _check_kw(kw)
    times = [float(v) for v in torch.as_tensor(times, dtype=torch.float32).reshape(-1).tolist()]
    if space not in ("field", "world"):
        raise L.RdrfError(f"space must be \"field\" or \"world\", not {space!r}")

    @torch.no_grad()
    def meshes():
        if not times:
            return
        alpha, _ = field.getDenseAlpha(gridSize, times=times)
        for k in range(len(times)):
            yield _mesh_of_slice(field, alpha, k, level, space, H, W, focal, kw)

    return meshes()


# ---- vertex colours: the appearance head at the vertices (fields.TensorBase.query_points, csrc/rdrf_point.hip) --------------
@torch.no_grad()
def vertex_colors(field, verts, t=None, view=(0, 0, 1)):
    """[nv,3] uint8 colours of FIELD-SPACE vertices (what field_mesh(space="field") returns): the field's rgb at each vertex
    at time t, seen along the one direction `view` (used as given), quantised as round(clamp(rgb, 0, 1) * 255)."""
    if t is None and field.DYNAMIC:
        raise L.RdrfError("vertex_colors: the dynamic field's colours depend on the time: pass t")
    rgb = field.query_points(verts, None if t is None else float(t), tuple(float(v) for v in view), want=("rgb",))["rgb"]
    return torch.round(rgb.clamp(0.0, 1.0) * 255.0).to(torch.uint8)


@torch.no_grad()
def colored_mesh(field, t=None, level=0.005, gridSize=None, view=(0, 0, 1), space="field", H=None, W=None, focal=None,
                 normals=False, flip=False, cap=False, simplify=None):
    """field_mesh with colours: (verts, faces[, normals], colors [nv,3] uint8).  The colours are those of the field-space
    vertices (vertex_colors), taken before any NDC2world mapping, so space="world" moves the vertices and keeps the colours.
    simplify=K clusters the coloured mesh: a cluster's colour is the mean of its members' colours."""
    if space not in ("field", "world"):
        raise L.RdrfError(f"space must be \"field\" or \"world\", not {space!r}")
    if t is None and field.DYNAMIC:
        raise L.RdrfError("field_mesh: the dynamic field's alpha depends on the time: pass t")
    alpha, _ = field.getDenseAlpha(gridSize, times=[0.0 if t is None else float(t)])
    kw = dict(normals=normals, flip=flip, cap=cap)
    if simplify is not None:
        kw["simplify"] = simplify
    return _mesh_of_slice(field, alpha, 0, level, space, H, W, focal, kw, color=lambda verts: vertex_colors(field, verts, t, view))


# ---- whole-scene meshes: the isosurface of the composed alpha volume (alpha.scene_dense_alpha, csrc/rdrf_scene_alpha.hip) ---
def _scene_t(t, who):
    if t is None:
        raise L.RdrfError(f"{who}: the scene's alpha depends on the time: pass t")
    return float(t)


@torch.no_grad()
def scene_mesh(tensorf_static, tensorf, t=None, level=0.005, gridSize=None, space="field", H=None, W=None, focal=None, **kw):
    """field_mesh of the whole scene at time t: scene_dense_alpha(gridSize, times=[t]) -> extract_isosurface.  The lattice and
    the box are the dynamic field's; kw as field_mesh: normals, flip, cap, simplify."""
    from .alpha import scene_dense_alpha
    _check_kw(kw)
    t = _scene_t(t, "scene_mesh")
    alpha, _ = scene_dense_alpha(tensorf_static, tensorf, gridSize, times=[t])
    return _mesh_of_slice(tensorf, alpha, 0, level, space, H, W, focal, kw)


def scene_mesh_sequence(tensorf_static, tensorf, times, level=0.005, gridSize=None, space="field", H=None, W=None, focal=None, **kw):
    """mesh_sequence of the whole scene: an iterator of one mesh per time from a single scene_dense_alpha over all times.  The
    arguments are checked here, at the call, not at the first next()."""
    from .alpha import check_scene_fields, scene_dense_alpha
    _check_kw(kw)
    check_scene_fields(tensorf_static, tensorf, "scene_mesh_sequence")
    times = [float(v) for v in torch.as_tensor(times, dtype=torch.float32).reshape(-1).tolist()]
    if space not in ("field", "world"):
        raise L.RdrfError(f"space must be \"field\" or \"world\", not {space!r}")

    @torch.no_grad()
    def meshes():
        if not times:
            return
        alpha, _ = scene_dense_alpha(tensorf_static, tensorf, gridSize, times=times)
        for k in range(len(times)):
            yield _mesh_of_slice(tensorf, alpha, k, level, space, H, W, focal, kw)

    return meshes()


@torch.no_grad()
def scene_vertex_colors(tensorf_static, tensorf, verts, t=None, view=(0, 0, 1)):
    """[nv,3] uint8 colours of FIELD-SPACE vertices of a scene mesh: rgb = o rgb_d + (1 - o) rgb_s with rgb_d / rgb_s the two
    fields' query_points colours at the vertex (time t, the one direction `view` used as given) and o the `owner` of
    scene_alpha_volume there; quantised as vertex_colors does."""
    from .alpha import scene_alpha_volume
    t = _scene_t(t, "scene_vertex_colors")
    view = tuple(float(v) for v in view)
    o = scene_alpha_volume(tensorf_static, tensorf, verts, [t], want=("owner",))["owner"]
    rgb_d = tensorf.query_points(verts, t, view, want=("rgb",))["rgb"]
    rgb_s = tensorf_static.query_points(verts, None, view, want=("rgb",))["rgb"]
    rgb = o * rgb_d + (1.0 - o) * rgb_s
    return torch.round(rgb.clamp(0.0, 1.0) * 255.0).to(torch.uint8)


@torch.no_grad()
def colored_scene_mesh(tensorf_static, tensorf, t=None, level=0.005, gridSize=None, view=(0, 0, 1), space="field", H=None, W=None,
                       focal=None, normals=False, flip=False, cap=False, simplify=None):
    """colored_mesh of the whole scene: (verts, faces[, normals], colors [nv,3] uint8), the colours (scene_vertex_colors) taken
    on the unsimplified field-space mesh, before clustering and before any NDC2world mapping."""
    from .alpha import scene_dense_alpha
    if space not in ("field", "world"):
        raise L.RdrfError(f"space must be \"field\" or \"world\", not {space!r}")
    t = _scene_t(t, "colored_scene_mesh")
    kw = dict(normals=normals, flip=flip, cap=cap)
    if simplify is not None:
        kw["simplify"] = simplify
    _check_kw(kw)
    alpha, _ = scene_dense_alpha(tensorf_static, tensorf, gridSize, times=[t])
    return _mesh_of_slice(tensorf, alpha, 0, level, space, H, W, focal, kw,
                          color=lambda verts: scene_vertex_colors(tensorf_static, tensorf, verts, t, view))


# ---- texture atlases: the field per texel of a per-face atlas (csrc/rdrf_bake.hip; DESIGN.md, "Texture atlases") -------------
def _texels(texels, who):
    if isinstance(texels, bool) or not isinstance(texels, int) or not L.BAKE_TEXELS_MIN <= texels <= L.BAKE_TEXELS_MAX:
        raise L.RdrfError(f"{who}: texels must be a whole number from {L.BAKE_TEXELS_MIN} to {L.BAKE_TEXELS_MAX}, not {texels!r}")
    return texels


def atlas_layout(n_faces, texels=8, width=None):
    """(Wt, Ht, R) of the atlas of n_faces faces: squares of texels x texels, two faces to a square, R = Wt // texels squares
    to a row, Ht = texels * ceil(ceil(n_faces / 2) / R).  width=None: the smallest power of two that holds
    ceil(sqrt(ceil(n_faces / 2))) squares side by side; a given width must hold one square."""
    q = _texels(texels, "atlas_layout")
    F = int(n_faces)
    if F < 0:
        raise L.RdrfError(f"atlas_layout: {F} faces")
    nsq = (F + 1) // 2
    if width is None:
        side = math.isqrt(nsq)
        need = q * max(1, side if side * side == nsq else side + 1)
        Wt = 1 << (need - 1).bit_length()
    else:
        if isinstance(width, bool) or not isinstance(width, int) or width < q:
            raise L.RdrfError(f"atlas_layout: an atlas {width!r} texels wide holds no square of {q}")
        Wt = width
    R = Wt // q
    return Wt, q * (-(-nsq // R)), R


def atlas_uv(n_faces, texels=8, width=None, device=None):
    """[n_faces,3,2] float32: the texture coordinates of every face's three corners, in the order of its vertices, u to the
    right and v up the array's rows (write_obj writes row y of the texture at image row Ht - 1 - y).  The corners sit on
    texel centres half a texel inside the face's half of its square, so a bilinear fetch inside the triangle stays on the
    face's own texels."""
    q = _texels(texels, "atlas_uv")
    Wt, Ht, R = atlas_layout(n_faces, q, width)
    f = np.arange(int(n_faces), dtype=np.int64)
    s, upper = f >> 1, (f & 1).astype(bool)
    lower_c = np.array([[0.5, 0.5], [q - 1.5, 0.5], [0.5, q - 1.5]])
    upper_c = np.array([[q - 0.5, q - 0.5], [2.5, q - 0.5], [q - 0.5, 2.5]])
    local = np.where(upper[:, None, None], upper_c[None], lower_c[None])
    origin = np.stack(((s % R) * q, (s // R) * q), -1).astype(np.float64)
    uv = (origin[:, None, :] + local) / np.array([Wt, max(Ht, 1)], dtype=np.float64)
    return torch.from_numpy(uv.astype(np.float32)).to("cpu" if device is None else device)


def _bake_mesh(verts, faces, who):
    """the checks of a mesh whose faces index the kernels' reads: shapes, types, and every index inside [0, nv) (one host read)"""
    if not torch.is_tensor(verts) or verts.dim() != 2 or verts.shape[1] != 3 or verts.dtype != torch.float32:
        raise L.RdrfError(f"{who}: verts must be a [nv,3] float32 tensor")
    if not torch.is_tensor(faces) or faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype != torch.int32:
        raise L.RdrfError(f"{who}: faces must be a [F,3] int32 tensor")
    if faces.shape[0] > 0:
        lo, hi = int(faces.min()), int(faces.max())
        if lo < 0 or hi >= verts.shape[0]:
            raise L.RdrfError(f"{who}: face indices run from {lo} to {hi}, the mesh has {verts.shape[0]} vertices")
    L.require_device(verts, faces)
    if verts.device != faces.device:
        raise L.RdrfError(f"{who}: verts are on {verts.device} and faces on {faces.device}")
    return verts.contiguous(), faces.contiguous()


def _bake_view(view, who):
    """None for "normal" (the kernels then look at each face along minus its normal), else a host array of three floats"""
    if isinstance(view, str):
        if view != "normal":
            raise L.RdrfError(f"{who}: view must be three numbers or \"normal\", not {view!r}")
        return None
    v = [float(x) for x in view]
    if len(v) != 3:
        raise L.RdrfError(f"{who}: view must be three numbers or \"normal\", not {view!r}")
    return (C.c_float * 3)(*v)


def _bake_fill(fill, who):
    """the colour of the texels no face owns: three whole numbers from 0 to 255, as a host array of three bytes"""
    v = list(fill) if isinstance(fill, (tuple, list)) or torch.is_tensor(fill) or isinstance(fill, np.ndarray) else None
    if v is None or len(v) != 3 or not all(float(x) == int(x) and 0 <= int(x) <= 255 for x in v):
        raise L.RdrfError(f"{who}: fill must be three whole numbers from 0 to 255, not {fill!r}")
    return (C.c_ubyte * 3)(*[int(x) for x in v])


@torch.no_grad()
def bake_texels(verts, faces, texels=8, width=None, view=(0, 0, 1)):
    """The geometry stage of a bake: dict(points [Ht,Wt,3], viewdirs [Ht,Wt,3], face [Ht,Wt] int32) over the atlas
    atlas_layout(F, texels, width).  points: where each texel lies on its face (FIELD-SPACE verts in, field-space points
    out); viewdirs: `view` as given, or with view="normal" minus the unit normal of the texel's face ((0, 0, 1) for a face
    without one); face: the owning face, -1 where there is none (points 0 there).  query_points at these points bakes any
    quantity of a field."""
    who = "bake_texels"
    q = _texels(texels, who)
    Wt, Ht, _ = atlas_layout(int(faces.shape[0]) if torch.is_tensor(faces) and faces.dim() == 2 else 0, q, width)
    view_c = _bake_view(view, who)
    verts, faces = _bake_mesh(verts, faces, who)
    dev = verts.device
    out = {"points": torch.empty(Ht, Wt, 3, device=dev), "viewdirs": torch.empty(Ht, Wt, 3, device=dev),
           "face": torch.empty(Ht, Wt, dtype=torch.int32, device=dev)}
    L.check(L.lib.rdrf_bake_texels(L.ptr(verts), L.ptr(faces), int(faces.shape[0]), q, Wt, Ht, view_c, L.ptr(out["points"]),
                                   L.ptr(out["viewdirs"]), L.ptr(out["face"]), L.stream_of(verts)), "rdrf_bake_texels")
    return out


@torch.no_grad()
def bake_texture(field, verts, faces, t=None, texels=8, width=None, view=(0, 0, 1), fill=(0, 0, 0), static=None, _chunk=None):
    """(texture [Ht,Wt,3] uint8, uv [F,3,2] float32): the field's colour per texel of the atlas of a FIELD-SPACE mesh,
    round(clamp(rgb, 0, 1) * 255) of query_points at the points and directions bake_texels gives, bit for bit; texels no face
    owns are `fill`.  static=: `field` is the dynamic field and the colours are the whole scene's, o rgb_d + (1 - o) rgb_s as
    in scene_vertex_colors.  t is required for the dynamic field and for the scene.  The texels are evaluated in chunks of
    whole squares (at most _chunk points), so the scratch does not grow with the atlas."""
    from ._params import field_structs
    who = "bake_texture"
    q = _texels(texels, who)
    Wt, Ht, _ = atlas_layout(int(faces.shape[0]) if torch.is_tensor(faces) and faces.dim() == 2 else 0, q, width)
    view_c = _bake_view(view, who)
    fill_c = _bake_fill(fill, who)
    limit = L.QUERY_POINTS_MAX if _chunk is None else int(_chunk)
    if not q * q <= limit <= L.QUERY_POINTS_MAX:
        raise L.RdrfError(f"{who}: chunks of {limit} points, a chunk holds one square of {q * q} texels to {L.QUERY_POINTS_MAX} points")
    if static is not None:
        from .alpha import check_scene_fields
        check_scene_fields(static, field, who)
        t = _scene_t(t, who)
    elif field.DYNAMIC:
        if t is None:
            raise L.RdrfError(f"{who}: the dynamic field's colours depend on the time: pass t")
        t = float(t)
    verts, faces = _bake_mesh(verts, faces, who)
    dev, F = verts.device, int(faces.shape[0])
    if dev != field.aabb.device:
        raise L.RdrfError(f"{who}: the mesh is on {dev} and the field on {field.aabb.device}")
    squares = max(1, min(limit // (q * q), (F + 1) // 2))
    tex = torch.empty(Ht, Wt, 3, dtype=torch.uint8, device=dev)
    uv = atlas_uv(F, q, Wt, device=dev)
    t_dev = None if t is None else torch.full((1,), t, dtype=torch.float32, device=dev)
    ws = L.workspace(dev, L.lib.rdrf_bake_ws_bytes(int(static is not None), int(field.DYNAMIC), q, squares))
    P, cfg = field_structs(field, field._param_list(), "ndc")
    common = (L.ptr(verts), L.ptr(faces), F, q, Wt, Ht, view_c, L.ptr(t_dev))
    tail = (fill_c, squares, L.ptr(tex), L.ptr(ws), ws.numel(), L.stream_of(verts))
    if static is None:
        L.check(L.lib.rdrf_bake_texture(C.byref(P), int(field.DYNAMIC), C.byref(cfg), *common, *tail), "rdrf_bake_texture")
    else:
        PS, cs = field_structs(static, static._param_list(), "ndc")
        ms, md = (None if f.alphaMask is None else f.alphaMask._struct() for f in (static, field))   # as scene_vertex_colors
        L.check(L.lib.rdrf_bake_scene_texture(C.byref(PS), C.byref(cs), C.byref(P), C.byref(cfg), *common, float(field._step_host),
                                              None if ms is None else C.byref(ms), None if md is None else C.byref(md), *tail),
                "rdrf_bake_scene_texture")
    return tex, uv


@torch.no_grad()
def textured_mesh(field, t=None, level=0.005, gridSize=None, texels=8, view=(0, 0, 1), space="field", H=None, W=None, focal=None,
                  normals=False, flip=False, cap=False, simplify=None, static=None):
    """field_mesh (static=: scene_mesh, `field` the dynamic field) with a texture atlas: (verts, faces[, normals], uv, texture).
    The texture is baked (bake_texture) on the final field-space mesh -- after simplify=K, so its resolution does not shrink
    with the vertex count, and before any NDC2world mapping: space="world" moves the vertices and keeps uv and texels."""
    if space not in ("field", "world"):
        raise L.RdrfError(f"space must be \"field\" or \"world\", not {space!r}")
    if space == "world" and (H is None or W is None or focal is None):   # before the volume, the meshing and the bake
        raise L.RdrfError("space=\"world\" maps NDC vertices through NDC2world and needs H, W and focal")
    _texels(texels, "textured_mesh")
    _bake_view(view, "textured_mesh")
    kw = dict(normals=normals, flip=flip, cap=cap)
    if simplify is not None:
        kw["simplify"] = simplify
    _check_kw(kw)
    if static is not None:
        from .alpha import scene_dense_alpha
        t = _scene_t(t, "textured_mesh")
        alpha, _ = scene_dense_alpha(static, field, gridSize, times=[t])
    else:
        if t is None and field.DYNAMIC:
            raise L.RdrfError("textured_mesh: the dynamic field's alpha depends on the time: pass t")
        alpha, _ = field.getDenseAlpha(gridSize, times=[0.0 if t is None else float(t)])
    mesh = _mesh_of_slice(field, alpha, 0, level, "field", None, None, None, kw)
    verts, faces = mesh[0], mesh[1]
    texture, uv = bake_texture(field, verts, faces, t, texels, None, view, static=static)
    world, wn = _to_world(field, verts, faces, space, H, W, focal)
    out = (world, faces) if not normals else (world, faces, (mesh[2] if wn is None else wn))
    return out + (uv, texture)


# ---- PLY (binary little-endian), numpy only ----------------------------------------------------------------------------
def _np(x, dtype):
    if torch.is_tensor(x):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(x), dtype=dtype)


def _vertex_dtype(normals, colors):
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if normals:
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    if colors:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    return np.dtype(fields)


def write_ply(path, verts, faces=None, normals=None, colors=None):
    """vertex: x y z [nx ny nz] [red green blue]; face: vertex_indices as uchar count + int indices.  faces=None: a point
    cloud, a vertex-only file without a face element."""
    v = _np(verts, "<f4").reshape(-1, 3)
    f = None if faces is None else _np(faces, "<i4").reshape(-1, 3)
    vd = _vertex_dtype(normals is not None, colors is not None)
    rec = np.zeros(len(v), dtype=vd)
    rec["x"], rec["y"], rec["z"] = v[:, 0], v[:, 1], v[:, 2]
    if normals is not None:
        n = _np(normals, "<f4").reshape(-1, 3)
        rec["nx"], rec["ny"], rec["nz"] = n[:, 0], n[:, 1], n[:, 2]
    if colors is not None:
        c = _np(colors, "u1").reshape(-1, 3)
        rec["red"], rec["green"], rec["blue"] = c[:, 0], c[:, 1], c[:, 2]
    kinds = {"<f4": "float", "|u1": "uchar"}
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}"]
    header += [f"property {kinds[vd[name].str]} {name}" for name in vd.names]
    if f is not None:
        frec = np.zeros(len(f), dtype=np.dtype([("n", "u1"), ("idx", "<i4", (3,))]))
        frec["n"], frec["idx"] = 3, f
        header += [f"element face {len(f)}", "property list uchar int vertex_indices"]
    header += ["end_header"]
    with open(path, "wb") as out:
        out.write(("\n".join(header) + "\n").encode("ascii"))
        out.write(rec.tobytes())
        if f is not None:
            out.write(frec.tobytes())


def read_ply(path):
    """what write_ply writes -> dict(verts [nv,3] f32, faces [nf,3] i32, normals / colors or None); a vertex-only file (a
    point cloud) comes back with an empty face array"""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")
    if lines[:2] != ["ply", "format binary_little_endian 1.0"]:
        raise ValueError(f"{path}: not a binary little-endian PLY")
    nv = nf = None
    props = []
    for line in lines[2:]:
        w = line.split()
        if w[:2] == ["element", "vertex"]:
            nv = int(w[2])
        elif w[:2] == ["element", "face"]:
            nf = int(w[2])
        elif w[:1] == ["property"] and nf is None:
            props.append(w[2])
    names = tuple(props)
    has_n, has_c = "nx" in names, "red" in names
    vd = _vertex_dtype(has_n, has_c)
    if names != vd.names:
        raise ValueError(f"{path}: vertex properties {names} are not what write_ply writes")
    rec = np.frombuffer(data, dtype=vd, count=nv, offset=end)
    nf = nf or 0
    frec = np.frombuffer(data, dtype=np.dtype([("n", "u1"), ("idx", "<i4", (3,))]), count=nf, offset=end + nv * vd.itemsize)
    if nf and not (frec["n"] == 3).all():
        raise ValueError(f"{path}: only triangles are read")
    stack = lambda keys, dt: np.stack([rec[k] for k in keys], -1).astype(dt) if nv else np.zeros((0, 3), dtype=dt)
    return {"verts": stack(("x", "y", "z"), np.float32), "faces": np.array(frec["idx"], dtype=np.int32).reshape(-1, 3),
            "normals": stack(("nx", "ny", "nz"), np.float32) if has_n else None,
            "colors": stack(("red", "green", "blue"), np.uint8) if has_c else None}


# ---- OBJ + MTL + PNG: a textured mesh as three files, standard library and numpy only ------------------------------------------
def _png_chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def write_png(path, image):
    """image [H,W,3] uint8, row 0 at the top: an 8-bit RGB PNG, every scanline with filter 0"""
    img = _np(image, "u1")
    if img.ndim != 3 or img.shape[2] != 3 or img.shape[0] < 1 or img.shape[1] < 1:
        raise L.RdrfError(f"write_png: the image must be [H,W,3] with H, W >= 1, not {img.shape}")
    Hh, Ww = img.shape[:2]
    rows = np.zeros((Hh, 1 + Ww * 3), dtype=np.uint8)
    rows[:, 1:] = img.reshape(Hh, Ww * 3)
    with open(path, "wb") as out:
        out.write(b"\x89PNG\r\n\x1a\n" + _png_chunk(b"IHDR", struct.pack(">IIBBBBB", Ww, Hh, 8, 2, 0, 0, 0))
                  + _png_chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + _png_chunk(b"IEND", b""))


def read_png(path):
    """what write_png writes -> [H,W,3] uint8 (8-bit RGB, filter 0 on every scanline; anything else is refused)"""
    with open(path, "rb") as f:
        data = f.read()
    if data[:8] != b"\x89PNG\r\n\x1a\n":
        raise ValueError(f"{path}: not a PNG")
    pos, idat, head = 8, b"", None
    while pos < len(data):
        n, kind = struct.unpack(">I", data[pos:pos + 4])[0], data[pos + 4:pos + 8]
        body = data[pos + 8:pos + 8 + n]
        if kind == b"IHDR":
            head = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat += body
        pos += 12 + n
    if head is None or head[2:] != (8, 2, 0, 0, 0):
        raise ValueError(f"{path}: only 8-bit RGB without interlacing is read")
    Ww, Hh = head[:2]
    rows = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(Hh, 1 + Ww * 3)
    if rows[:, 0].any():
        raise ValueError(f"{path}: only scanlines with filter 0 are read")
    return np.ascontiguousarray(rows[:, 1:]).reshape(Hh, Ww, 3)


def _obj_paths(path):
    base = os.path.splitext(os.fspath(path))[0]
    return base + ".obj", base + ".mtl", base + ".png"


def write_obj(path, verts, faces, uv, texture, normals=None):
    """A textured mesh as <base>.obj (v, vt -- three per face --, optional vn, f a/ta[/na] ...), <base>.mtl (map_Kd) and
    <base>.png, <base> = path without its suffix.  uv [F,3,2] and texture [Ht,Wt,3] uint8 as bake_texture returns them: row y
    of the texture is written at image row Ht - 1 - y (OBJ's v runs upwards).  Floats are written with nine significant
    digits, which read_obj reads back to the same float32.  Returns the three paths."""
    v = _np(verts, "<f4").reshape(-1, 3)
    f = _np(faces, "<i4").reshape(-1, 3)
    vt = _np(uv, "<f4").reshape(-1, 2)
    tex = _np(texture, "u1")
    n = None if normals is None else _np(normals, "<f4").reshape(-1, 3)
    if vt.shape[0] != 3 * f.shape[0]:
        raise L.RdrfError(f"write_obj: uv must be [F,3,2] for the {f.shape[0]} faces, not {np.shape(uv)}")
    if tex.ndim != 3 or tex.shape[2] != 3 or tex.shape[0] < 1 or tex.shape[1] < 1:
        raise L.RdrfError(f"write_obj: the texture must be [Ht,Wt,3] uint8 with texels in it (an empty mesh has no atlas), not {tex.shape}")
    obj, mtl, png = _obj_paths(path)
    write_png(png, tex[::-1])
    with open(mtl, "w") as out:
        out.write(f"newmtl baked\nKa 0 0 0\nKd 1 1 1\nKs 0 0 0\nillum 0\nmap_Kd {os.path.basename(png)}\n")
    lines = [f"mtllib {os.path.basename(mtl)}", "usemtl baked"]
    lines += ["v %.9g %.9g %.9g" % tuple(r) for r in v.tolist()]
    lines += ["vt %.9g %.9g" % tuple(r) for r in vt.tolist()]
    if n is not None:
        lines += ["vn %.9g %.9g %.9g" % tuple(r) for r in n.tolist()]
    fmt = "f %d/%d %d/%d %d/%d" if n is None else "f %d/%d/%d %d/%d/%d %d/%d/%d"
    corners = np.stack((f + 1, 3 * np.arange(len(f))[:, None] + np.arange(1, 4)[None]) + (() if n is None else (f + 1,)), -1)
    lines += [fmt % tuple(r) for r in corners.reshape(len(f), -1).tolist()]
    with open(obj, "w") as out:
        out.write("\n".join(lines) + "\n")
    return obj, mtl, png


def read_obj(path):
    """what write_obj writes -> dict(verts [nv,3] f32, faces [F,3] i32, uv [F,3,2] f32, normals [nv,3] f32 or None, texture
    [Ht,Wt,3] uint8 with the row flip undone, mtl: the material file's text)"""
    obj, _, _ = _obj_paths(path)
    v, vt, vn, f, ft, mtllib = [], [], [], [], [], None
    with open(obj) as src:
        for line in src:
            w = line.split()
            if not w:
                continue
            if w[0] == "v":
                v.append([float(x) for x in w[1:4]])
            elif w[0] == "vt":
                vt.append([float(x) for x in w[1:3]])
            elif w[0] == "vn":
                vn.append([float(x) for x in w[1:4]])
            elif w[0] == "f":
                if len(w) != 4:
                    raise ValueError(f"{obj}: only triangles are read")
                c = [x.split("/") for x in w[1:]]
                f.append([int(x[0]) - 1 for x in c])
                ft.append([int(x[1]) - 1 for x in c])
            elif w[0] == "mtllib":
                mtllib = w[1]
    if mtllib is None:
        raise ValueError(f"{obj}: no mtllib")
    with open(os.path.join(os.path.dirname(obj), mtllib)) as src:
        mtl = src.read()
    maps = [line.split()[1] for line in mtl.split("\n") if line.split()[:1] == ["map_Kd"]]
    if len(maps) != 1:
        raise ValueError(f"{mtllib}: one map_Kd is read, not {len(maps)}")
    arr = lambda x, dt, cols: np.asarray(x, dtype=dt).reshape(-1, cols)
    vt, ft = arr(vt, np.float32, 2), arr(ft, np.int32, 3)
    return {"verts": arr(v, np.float32, 3), "faces": arr(f, np.int32, 3), "uv": vt[ft.reshape(-1)].reshape(-1, 3, 2),
            "normals": arr(vn, np.float32, 3) if vn else None,
            "texture": np.ascontiguousarray(read_png(os.path.join(os.path.dirname(obj), maps[0]))[::-1]), "mtl": mtl}


def load_field(path, device="cuda"):
    """the reload recipe of train.py:433-447 on this package's classes; the class is told from the state dict"""
    from .fields import TensorVMSplit, TensorVMSplit_TimeEmbedding
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    kwargs = dict(ckpt["kwargs"])
    kwargs.pop("se3_poses", None)
    kwargs.pop("focal_ratio_refine", None)
    kwargs.update({"device": device})
    cls = TensorVMSplit_TimeEmbedding if "density_layer1.weight" in ckpt["state_dict"] else TensorVMSplit
    field = cls(**kwargs)
    field.load(ckpt)
    return field


@torch.no_grad()
def export_mesh(field_or_ckpt_path, ply_path, t=None, level=0.005, gridSize=None, space="field", H=None, W=None, focal=None,
                device="cuda", color_view=None, static=None, texture=None, **kw):
    """train.py:107-118: the field (or the checkpoint at a path) -> dense alpha -> isosurface -> PLY.  Returns the mesh.
    color_view: a view direction; the PLY then carries the vertex colours of colored_mesh, which come last in the mesh.
    static: the static field (or its checkpoint's path) next to a dynamic `field_or_ckpt_path`: the mesh is then the whole
    scene's (scene_mesh / colored_scene_mesh) at time t.  kw: normals, flip, cap, simplify.
    texture=q: a textured mesh (textured_mesh, squares of q texels) goes to an OBJ, an MTL and a PNG instead (write_obj; the
    suffix of ply_path is replaced); color_view is then the bake's view direction, three numbers (default (0, 0, 1)) or
    "normal"."""
    is_path = lambda f: isinstance(f, (str, bytes)) or hasattr(f, "__fspath__")
    if texture is not None:   # refused before a checkpoint is loaded
        _check_kw(kw)
        _texels(texture, "export_mesh")
    elif isinstance(color_view, str):
        raise L.RdrfError("export_mesh: color_view=\"normal\" is a direction per texel: it needs texture=")
    field = load_field(field_or_ckpt_path, device) if is_path(field_or_ckpt_path) else field_or_ckpt_path
    if texture is not None:
        st = load_field(static, device) if static is not None and is_path(static) else static
        out = textured_mesh(field, t, level, gridSize, texture, (0, 0, 1) if color_view is None else color_view, space, H, W, focal,
                            static=st, **kw)
        write_obj(ply_path, out[0], out[1], out[-2], out[-1], normals=out[2] if len(out) > 4 else None)
        return out
    if static is not None:
        _check_kw(kw)
        st = load_field(static, device) if is_path(static) else static
        if color_view is None:
            out = scene_mesh(st, field, t, level, gridSize, space, H, W, focal, **kw)
            write_ply(ply_path, out[0], out[1], normals=out[2] if len(out) > 2 else None)
        else:
            out = colored_scene_mesh(st, field, t, level, gridSize, color_view, space, H, W, focal, **kw)
            write_ply(ply_path, out[0], out[1], normals=out[2] if len(out) > 3 else None, colors=out[-1])
        return out
    if color_view is None:
        out = field_mesh(field, t, level, gridSize, space, H, W, focal, **kw)
        write_ply(ply_path, out[0], out[1], normals=out[2] if len(out) > 2 else None)
        return out
    _check_kw(kw)
    out = colored_mesh(field, t, level, gridSize, color_view, space, H, W, focal, **kw)
    write_ply(ply_path, out[0], out[1], normals=out[2] if len(out) > 3 else None, colors=out[-1])
    return out
