"""GPU tests of the whole-scene volumes (csrc/rdrf_scene_alpha.hip, alpha.scene_alpha_volume / scene_dense_alpha,
mesh.scene_mesh / scene_mesh_sequence / scene_vertex_colors / colored_scene_mesh, export_mesh(static=)): the components bit
for bit against query_points and alpha_volume, alpha and owner against the float64 reference of tests/_scene_prim.py on those
component bits inside its bounds, the contract of the entry point, and the Python layer on top."""
import math

import numpy as np
import pytest
import torch

import _scene_prim as P
from _gpu_util import COMMON
from _twin import CHILD, assert_same_dict, run_twin, same_bits
from _util import pkg, record_margin

pytestmark = pytest.mark.gpu
DEV = "cuda"
GRID, T = [9, 11, 7], 3
AABB = torch.tensor([[-1.5, -1.67, -1.0], [1.5, 1.67, 1.0]])
AABB_S = AABB * torch.tensor([[0.9], [0.8]])   # the static field has a box of its own: each field normalises with its own
LENGTH = 0.4
ALL = P.ORDER
_cache = {}


def build_fields(act):
    """fresh fields on the suite's small grid, tSize 3, conditioned so that both sigmas spread over (0, a few), the blending
    over most of (0, 1) and the warp moves the points (density_shift 0: softplus sigma of order 1, not e^-10)"""
    import rodynrf
    torch.manual_seed(11)
    kw = dict(COMMON, near_far=[0.0, 1.0], density_shift=0.0, fea2denseAct=act)
    st = rodynrf.TensorVMSplit(AABB_S, GRID, T, DEV, shadingMode="MLP_Fea", fea_pe=2, **kw)
    dy = rodynrf.TensorVMSplit_TimeEmbedding(AABB, GRID, T, DEV, shadingMode="MLP_Fea_late_view", fea_pe=0, **kw)
    with torch.no_grad():
        for p in list(st.density_line) + list(dy.density_line) + list(dy.blending_line):
            p.mul_(6.0)
        dy.density_layer2.weight.mul_(4.0)
        dy.blending_layer2.weight.mul_(12.0)
    return st, dy


def fields(act="relu"):
    if act not in _cache:
        _cache[act] = build_fields(act)
    return _cache[act]


def points(M, seed, spread=1.04):
    """spread 1.04: a little beyond the dynamic box, well beyond the static one"""
    g = torch.Generator().manual_seed(seed)
    c, h = (AABB[0] + AABB[1]) / 2, (AABB[1] - AABB[0]) / 2
    return (c + (torch.rand(M, 3, generator=g) * 2 - 1) * h * spread).to(DEV)


def times_of(Tn):
    return torch.tensor([0.25] if Tn == 1 else [-1.0, 0.3, 1.0][:Tn], device=DEV)


def scene(st, dy, xyz, times, want=ALL, **kw):
    return pkg("alpha").scene_alpha_volume(st, dy, xyz, times, LENGTH, want=want, **kw)


def components(st, dy, xyz, times):
    """sigma_s, sigma_d, blending [M,T] from the public point queries, a call per time"""
    ss = st.query_points(xyz, None, None, want=("sigma",))["sigma"]
    per_t = [dy.query_points(xyz, float(t), None, want=("sigma", "blending")) for t in times.cpu()]
    return {"sigma_s": ss[:, None].expand(-1, len(per_t)).contiguous(), "sigma_d": torch.stack([q["sigma"] for q in per_t], -1),
            "blending": torch.stack([q["blending"] for q in per_t], -1)}


def check_composite(tag, out, length=LENGTH):
    """alpha and owner against the float64 reference on the call's own component bits"""
    n = lambda k: out[k].cpu().numpy()
    wa, wo, ok = P.check(n("alpha"), n("owner"), n("sigma_s"), n("sigma_d"), n("blending"), np.float32(length))
    print(f"{tag}: alpha err / bound {wa:.3f}, owner err / bound {wo:.3f}")
    record_margin(f"{tag} alpha vs float64 reference", wa)
    record_margin(f"{tag} owner vs float64 reference", wo)
    assert ok and wa <= 1.0 and wo <= 1.0, (tag, wa, wo, ok)


def check_components(tag, out, ref):
    for k, v in ref.items():
        assert same_bits(out[k], v), (tag, k)


@pytest.mark.parametrize("act", ["relu", "softplus"])
def test_components_are_the_point_queries_bits_and_the_composite_is_in_bounds(act):
    st, dy = fields(act)
    for M in (0, 1, 31, 32, 33, 95):
        for Tn in (1, 3):
            xyz, times = points(M, 100 * M + Tn), times_of(Tn)
            out = scene(st, dy, xyz, times)
            assert sorted(out) == sorted(ALL) and all(v.shape == (M, Tn) for v in out.values())
            if M == 0:
                continue
            check_components(f"{act} M={M} T={Tn}", out, components(st, dy, xyz, times))
            check_composite(f"{act} M={M} T={Tn}", out)
            if M == 95:   # the case is not trivial: both fields, and a blending that is neither 0 nor 1
                assert float(out["sigma_s"].max()) > 0.1 and float(out["sigma_d"].max()) > 0.1
                assert float(out["blending"].min()) < 0.4 and float(out["blending"].max()) > 0.6
                assert 0.02 < float(out["owner"].mean()) < 0.98 and float(out["alpha"].max()) > 0.05


def test_points_outside_either_box_behave_as_the_point_queries_there():
    st, dy = fields("relu")
    xyz, times = points(333, 5, spread=2.0), times_of(3)   # about an eighth of the points inside the dynamic box
    inside = ((xyz >= AABB[0].to(DEV)) & (xyz <= AABB[1].to(DEV))).all(-1)
    assert 10 < int(inside.sum()) < 100
    out = scene(st, dy, xyz, times)
    check_components("outside", out, components(st, dy, xyz, times))
    check_composite("outside", out)


def test_masks_empty_a_field_as_compute_alpha_does():
    import rodynrf
    A = pkg("alpha")
    st, dy = fields("softplus")
    g = torch.Generator().manual_seed(5)
    m_s = rodynrf.AlphaGridMask(DEV, AABB_S, (torch.rand(7, 11, 9, T, generator=g) < 0.1).float(), T)
    m_d = rodynrf.AlphaGridMask(DEV, AABB, (torch.rand(5, 6, 4, T, generator=g) < 0.12).float(), T)
    xyz, times = points(333, 9), times_of(3)
    free = scene(st, dy, xyz, times, masks=None)
    for tag, ms, md in (("both", m_s, m_d), ("static only", m_s, None), ("dynamic only", None, m_d)):
        out = scene(st, dy, xyz, times, masks=(ms, md))
        assert same_bits(out["sigma_s"], A.alpha_volume(st, xyz, times, LENGTH, ms, want_sigma=True)[1]), tag
        assert same_bits(out["sigma_d"], A.alpha_volume(dy, xyz, times, LENGTH, md, want_sigma=True)[1]), tag
        assert same_bits(out["blending"], free["blending"]), tag   # the blending is not masked
        check_composite(f"masks {tag}", out)
        for k, m in (("sigma_s", ms), ("sigma_d", md)):
            if m is not None:
                dropped = int(((out[k] == 0) & (free[k] > 0)).sum())
                assert 50 < dropped < 950, (tag, k, dropped)
    assert st.alphaMask is None and dy.alphaMask is None
    st.alphaMask, dy.alphaMask = m_s, m_d
    try:
        by_field = scene(st, dy, xyz, times)   # masks="fields"
    finally:
        st.alphaMask, dy.alphaMask = None, None
    assert_same_dict(by_field, scene(st, dy, xyz, times, masks=(m_s, m_d)))


def test_a_call_whose_tile_queue_hands_out_further_rounds():
    """Launch geometry (csrc/rdrf_host.hpp geo_for_units): at most 256 workgroups of at most 8 waves, a wave per 32-point tile,
    so one launch holds 256 * 8 = 2048 tiles = 65 536 points at once; every tile beyond comes from the workgroup's queue
    (tile_queue_next).  M = 2^21 + 5 is 65 537 tiles -- 32 full rounds and one last tile of 5 points -- and T = 2 runs the T-loop
    in each.  The components are compared with the point queries (two calls, themselves queue-driven but with one time) and the
    composite with the float64 reference on all 4.2 M entries."""
    st, dy = fields("relu")
    M = (1 << 21) + 5
    assert M > 32 * 256 * 8
    xyz, times = points(M, 21), times_of(2)
    out = scene(st, dy, xyz, times)
    check_components("queue rounds", out, components(st, dy, xyz, times))
    check_composite("queue rounds", out)
    head = scene(st, dy, xyz[:100], times)
    tail = scene(st, dy, xyz[-37:], times)
    for k in ALL:
        assert same_bits(out[k][:100], head[k]) and same_bits(out[k][-37:], tail[k]), k


def _const_head(layer, value):
    layer.weight.zero_()
    layer.bias.fill_(value)


def test_seeded_edge_inputs():
    """weights and points set so that the edges are reached: b exactly 0, exactly 1 and at 2^-126 (2^-125.9: a normal number), one field empty, both empty
    (alpha and owner exactly 0), saturated sigma (alpha exactly 1), and a NaN in the static field's factors that reaches some
    points and not others"""
    xyz, times = points(200, 3), times_of(3)

    def run(tag, st, dy):
        out = scene(st, dy, xyz, times)
        check_components(tag, out, components(st, dy, xyz, times))
        check_composite(tag, out)
        return out

    st, dy = build_fields("relu")
    with torch.no_grad():
        _const_head(dy.blending_layer2, -200.0)
        o = run("b = 0", st, dy)
        assert bool((o["blending"] == 0).all()) and bool((o["owner"] == 0).all()) and float(o["alpha"].max()) > 0.05
        _const_head(dy.blending_layer2, 100.0)
        o = run("b = 1", st, dy)
        assert bool((o["blending"] == 1).all()) and bool((o["owner"][o["sigma_d"] > 1e-3] == 1).all())
        assert bool((o["owner"][o["sigma_d"] == 0] == 0).all())
        _const_head(dy.blending_layer2, -125.9 * math.log(2.0))   # the bottom of the normal range, clear of a flush to zero
        o = run("b = 2^-126", st, dy)
        assert 2.0 ** -126 <= float(o["blending"].min()) and float(o["blending"].max()) < 2.0 ** -125
        _const_head(dy.blending_layer2, 0.3)
        for p in st.density_line:
            p.zero_()
        o = run("static empty", st, dy)
        assert bool((o["sigma_s"] == 0).all()) and bool((o["owner"][o["sigma_d"] > 1e-3] == 1).all())
        _const_head(dy.density_layer2, -1.0)
        o = run("both empty", st, dy)
        assert bool((o["sigma_d"] == 0).all()) and bool((o["alpha"] == 0).all()) and bool((o["owner"] == 0).all())
        _const_head(dy.density_layer2, 1.0e4)
        _const_head(dy.blending_layer2, 100.0)
        o = run("saturated", st, dy)
        assert bool((o["alpha"] == 1).all()) and bool((o["owner"] == 1).all())
        st, dy = build_fields("softplus")   # softplus hands a NaN feature on (relu's fmaxf does not)
        st.density_line[0][0, 0, GRID[0] // 2, 0] = float("nan")
        o = run("NaN", st, dy)
        nan = torch.isnan(o["sigma_s"])
        assert 0 < int(nan.sum()) < nan.numel() and torch.equal(torch.isnan(o["alpha"]), nan) and torch.equal(torch.isnan(o["owner"]), nan)


def test_only_what_is_asked_for_is_written_and_alone_equals_together():
    st, dy = fields("softplus")
    M, pad = 95, 33
    xyz, times = points(M, 8), times_of(3)
    together = scene(st, dy, xyz, times)
    nan_bytes = lambda: torch.full(((M + pad) * 3 * 4,), 0xFF, dtype=torch.uint8, device=DEV).view(torch.float32).view(M + pad, 3)
    for want in [(k,) for k in ALL] + [("alpha", "owner"), ("sigma_s", "blending"), ("sigma_d", "blending"), ALL]:
        bufs = {k: nan_bytes() for k in ALL}
        got = scene(st, dy, xyz, times, want=want, _out={k: bufs[k][:M] for k in want})
        assert sorted(got) == sorted(want)
        for k in ALL:
            raw = bufs[k].view(torch.int32)
            if k in want:
                assert same_bits(bufs[k][:M], together[k]), (want, k)           # alone = together, bit for bit
                assert bool((raw[M:] == -1).all()), (want, k)                   # the padding past M keeps its NaN bytes
            else:
                assert bool((raw == -1).all()), (want, k)


def test_a_point_does_not_depend_on_its_batch_or_on_T():
    st, dy = fields("relu")
    xyz, times = points(165, 13), times_of(3)
    full = scene(st, dy, xyz, times)
    for lo, hi in ((0, 1), (5, 40), (33, 165)):
        for k in range(3):
            part = scene(st, dy, xyz[lo:hi].contiguous(), times[k:k + 1])
            for name in ALL:
                assert same_bits(part[name][:, 0], full[name][lo:hi, k]), (lo, hi, k, name)
    rev = scene(st, dy, xyz, times.flip(0))
    for name in ALL:
        assert same_bits(rev[name].flip(1), full[name]), name


def det_case():
    """the case both libraries run (tests/_det_child.py case)"""
    st, dy = fields("softplus")
    return scene(st, dy, points(165, 77), times_of(3))


def test_deterministic_library_gives_the_same_bits(tmp_path):
    ours = det_case()
    assert len(ours) == 5
    assert_same_dict(run_twin(tmp_path, [CHILD, "case", "test_gpu_scene_volume"], det=True), ours)


# ---- the Python layer ------------------------------------------------------------------------------------------------
def test_scene_dense_alpha_is_the_volume_call_on_its_lattice(monkeypatch):
    import rodynrf
    A = pkg("alpha")
    st, dy = fields("relu")
    monkeypatch.setattr(A, "SLAB_POINTS", 2 * GRID[1] * GRID[2])   # slabs of 2 rows: 9 = 4 x 2 + 1
    alpha, owner, dense = rodynrf.scene_dense_alpha(st, dy, want_owner=True)
    assert alpha.shape == owner.shape == (*GRID, T) and dense.shape == (*GRID, 3)
    assert torch.equal(dense, dy.getDenseAlpha()[1])               # the dynamic field's lattice
    times = A.lattice_times(T).to(DEV)
    ref = A.scene_alpha_volume(st, dy, dense.reshape(-1, 3), times, want=("alpha", "owner"))   # length: the dynamic field's step
    assert same_bits(alpha.reshape(-1, T), ref["alpha"]) and same_bits(owner.reshape(-1, T), ref["owner"])
    assert same_bits(ref["alpha"], A.scene_alpha_volume(st, dy, dense.reshape(-1, 3), times, dy._step_host)["alpha"])
    monkeypatch.setattr(A, "SLAB_POINTS", 1 << 21)
    whole, _ = rodynrf.scene_dense_alpha(st, dy)
    assert same_bits(whole, alpha) and float(alpha.max()) > 0.01
    a2, _ = rodynrf.scene_dense_alpha(st, dy, gridSize=(4, 5, 3), times=[-1.0, 0.25])
    assert a2.shape == (4, 5, 3, 2)


def _level(alpha):
    return float(alpha.flatten().kthvalue(int(alpha.numel() * 0.6)).values)


def test_scene_mesh_and_sequence_are_the_isosurface_of_that_volume():
    import rodynrf
    st, dy = fields("relu")
    ts = [-1.0, 0.3]
    alpha, _ = rodynrf.scene_dense_alpha(st, dy, times=ts)
    level = _level(alpha)
    seq = list(rodynrf.scene_mesh_sequence(st, dy, ts, level, normals=True))
    assert len(seq) == 2
    for k, t in enumerate(ts):
        want = rodynrf.extract_isosurface(alpha, level, dy.aabb, t_index=k, normals=True)
        one = rodynrf.scene_mesh(st, dy, t, level, normals=True)
        assert want[0].shape[0] > 20 and want[1].shape[0] > 20
        for a, b, c in zip(want, one, seq[k]):
            assert same_bits(a, b) and same_bits(a, c)
    capped = rodynrf.scene_mesh(st, dy, ts[0], level, cap=True, flip=True)
    want = rodynrf.extract_isosurface(alpha, level, dy.aabb, t_index=0, cap=True, flip=True)
    assert same_bits(capped[0], want[0]) and same_bits(capped[1], want[1])
    world = rodynrf.scene_mesh(st, dy, ts[0], level, space="world", H=270, W=480, focal=400.0)
    plain = rodynrf.scene_mesh(st, dy, ts[0], level)
    assert same_bits(world[0], pkg("mesh").ndc_to_world(plain[0], 270, 480, 400.0)) and same_bits(world[1], plain[1])
    assert list(rodynrf.scene_mesh_sequence(st, dy, [], level)) == []


def test_scene_vertex_colors_and_colored_scene_mesh():
    import rodynrf
    st, dy = fields("relu")
    t, view = 0.3, (0.0, 0.6, 0.8)
    alpha, _ = rodynrf.scene_dense_alpha(st, dy, times=[t])
    level = _level(alpha)
    verts, faces = rodynrf.scene_mesh(st, dy, t, level)
    col = rodynrf.scene_vertex_colors(st, dy, verts, t, view)
    o = rodynrf.scene_alpha_volume(st, dy, verts, [t], want=("owner",))["owner"]
    rgb_d = dy.query_points(verts, t, view, want=("rgb",))["rgb"]
    rgb_s = st.query_points(verts, None, view, want=("rgb",))["rgb"]
    want = torch.round((o * rgb_d + (1.0 - o) * rgb_s).clamp(0.0, 1.0) * 255.0).to(torch.uint8)
    assert col.dtype == torch.uint8 and col.shape == (verts.shape[0], 3) and torch.equal(col, want)
    assert 0.02 < float(o.mean()) < 0.98 and int(col.max()) > int(col.min())
    mesh = rodynrf.colored_scene_mesh(st, dy, t, level, view=view, normals=True)
    assert len(mesh) == 4 and same_bits(mesh[0], verts) and same_bits(mesh[1], faces) and torch.equal(mesh[3], col)
    simple = rodynrf.colored_scene_mesh(st, dy, t, level, view=view, simplify=2)
    lattice = rodynrf.simplify_lattice(dy.aabb, alpha.shape, 2)
    want = rodynrf.simplify_mesh(verts, faces, lattice["cell"], lattice["grid"], lattice["aabb"], colors=col)
    for a, b in zip(simple, want):
        assert same_bits(a, b)


def test_export_mesh_with_and_without_the_static_field(tmp_path):
    import rodynrf
    st, dy = fields("relu")
    t, view = 0.3, (0.0, 0.0, 1.0)
    level = _level(rodynrf.scene_dense_alpha(st, dy, times=[t])[0])
    path = str(tmp_path / "scene.ply")
    out = rodynrf.export_mesh(dy, path, t, level, static=st, normals=True, color_view=view)
    want = rodynrf.colored_scene_mesh(st, dy, t, level, view=view, normals=True)
    back = rodynrf.read_ply(path)
    for a, b, k in zip(out, want, ("verts", "faces", "normals", "colors")):
        assert same_bits(a, b) and np.array_equal(back[k], a.cpu().numpy()), k
    out = dy.export_mesh(path, t, level, static=st)            # the method form, no colours
    back = rodynrf.read_ply(path)
    assert same_bits(out[0], rodynrf.scene_mesh(st, dy, t, level)[0]) and back["colors"] is None and back["normals"] is None
    assert np.array_equal(back["verts"], out[0].cpu().numpy()) and np.array_equal(back["faces"], out[1].cpu().numpy())
    # the whole scene is not the dynamic field's own mesh
    own = rodynrf.field_mesh(dy, t, level)
    assert own[0].shape != out[0].shape or not torch.equal(own[0], out[0])
    # checkpoints by path, as tools/export_mesh.py --with-static hands them in
    ck_s, ck_d = str(tmp_path / "s.th"), str(tmp_path / "d.th")
    st.save(None, None, ck_s)
    dy.save(None, None, ck_d)
    by_path = rodynrf.export_mesh(ck_d, str(tmp_path / "p.ply"), t, level, static=ck_s, device=DEV)
    assert same_bits(by_path[0], out[0]) and same_bits(by_path[1], out[1])
    assert open(str(tmp_path / "p.ply"), "rb").read() == open(path, "rb").read()
    # without static= the file is what field_mesh + write_ply give, byte for byte, call after call
    files = [str(tmp_path / f"f{k}.ply") for k in range(3)]
    rodynrf.export_mesh(dy, files[0], t, level, normals=True)
    rodynrf.export_mesh(dy, files[1], t, level, normals=True)
    m = rodynrf.field_mesh(dy, t, level, normals=True)
    rodynrf.write_ply(files[2], m[0], m[1], normals=m[2])
    data = [open(f, "rb").read() for f in files]
    assert data[0] == data[1] == data[2] and len(data[0]) > 1000
