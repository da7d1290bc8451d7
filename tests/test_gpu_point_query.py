"""GPU tests of the point queries (csrc/rdrf_point.hip, fields.TensorBase.query_points, mesh.vertex_colors / colored_mesh).

The main test is the identity with forward(): a point queried with a sample's position, its ray's time and its ray's
normalised view direction gets the sample's bits -- sigma, blending and xyz_prime on every valid sample, rgb on every sample
the forward computed a colour for (weight > rayMarch_weight_thres).  The rest holds the query to the goldens, to itself under
permutation, sub-batching, chunking and the two time modes, to the float64 reference of tests/_point_prim.py for a view
direction that is not a unit vector, and the coloured meshes to field_mesh + vertex_colors."""

import pytest
import torch

from _point_prim import point_reference, ray_norm_viewdirs
from _twin import CHILD, assert_same_dict, run_twin, same_bits
from _util import FWD_ELEM, assert_close, pkg

pytestmark = pytest.mark.gpu

DEV = "cuda"
POINT_CASES = ["ndc_relu", "ndc_softplus", "contract_relu_te", "contract_softplus_te"]
OUTS = {"static": ("sigma", "rgb"), "dynamic": ("sigma", "rgb", "blending", "xyz_prime")}
LATTICE = (12, 10, 9)   # the fixture lattice of tests/test_gpu_iso.py

_cases = {}


def case(name):
    """a golden case once per session: the fields, the ray batch on the device, its samples as a point batch, the no-grad
    forward of both fields and the query of every sample point (all outputs)"""
    if name not in _cases:
        from _gpu_util import fields_from_case
        g, st, dy, (sd_s, cfg_s, sd_d, cfg_d) = fields_from_case(name, DEV)
        rt = str(g["meta.ray_type"])
        dv = lambda k: torch.from_numpy(g[k]).to(DEV)
        rays, ts, xyz, z, valid = dv("rays"), dv("ts"), dv("xyz"), dv("z"), dv("valid")
        N, S = z.shape
        c = dict(g=g, rt=rt, N=N, S=S, fields={"static": st, "dynamic": dy}, sd={"static": (sd_s, cfg_s), "dynamic": (sd_d, cfg_d)},
                 valid=valid.reshape(-1).bool(), pts=xyz.reshape(-1, 3).contiguous(),
                 t=ts[:, None].expand(N, S).reshape(-1).contiguous(),
                 vd=ray_norm_viewdirs(g["rays"]).to(DEV)[:, None, :].expand(N, S, 3).reshape(-1, 3).contiguous())
        with torch.no_grad():
            c["fwd"] = {w: f(rays, ts, None, xyz, z, valid, is_train=True, ray_type=rt, N_samples=S) for w, f in c["fields"].items()}
        c["query"] = {w: f.query_points(c["pts"], c["t"], c["vd"], want=OUTS[w]) for w, f in c["fields"].items()}
        _cases[name] = c
    return _cases[name]


# ---- 1. identity with forward -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["static", "dynamic"])
@pytest.mark.parametrize("name", POINT_CASES)
def test_query_is_the_forward_of_the_same_sample(name, which):
    c = case(name)
    field, o, q = c["fields"][which], c["fwd"][which], c["query"][which]
    v = c["valid"]
    assert int(v.sum()) >= 50
    assert same_bits(q["sigma"][v], o.sigma.reshape(-1)[v]), "sigma"
    if which == "dynamic":
        assert same_bits(q["blending"][v], o.blending.reshape(-1)[v]), "blending"
        assert same_bits(q["xyz_prime"][v], o.xyz_prime.reshape(-1, 3)[v]), "xyz_prime"
    m = (o.weight > field.rayMarch_weight_thres).reshape(-1)
    print(f"{name} {which}: {int(m.sum())} app-masked of {m.numel()} samples, {int(v.sum())} valid")
    assert int(m.sum()) >= 50 and bool(v[m].all())
    diff = (q["rgb"][m] != o.rgb.reshape(-1, 3)[m]).any(-1)
    assert not bool(diff.any()), f"rgb differs on {int(diff.sum())} of {int(m.sum())} samples, max " \
                                 f"{float((q['rgb'][m] - o.rgb.reshape(-1, 3)[m]).abs().max()):.3e}"
    assert same_bits(q["rgb"][m], o.rgb.reshape(-1, 3)[m]), "rgb"


# ---- 2. golden parity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", POINT_CASES)
def test_query_matches_the_goldens(name):
    """the tolerance tests/test_gpu_forward.py applies to the same arrays: 1e-4 of the array's max, and element-wise
    |err| <= 1e-4 |ref| + 1e-6 max|ref|; colours on the samples the reference computed one for, away from the threshold"""
    c = case(name)
    g, v = c["g"], c["valid"].cpu()
    for which, tag in (("static", "fs."), ("dynamic", "fd.")):
        q = c["query"][which]
        w = torch.from_numpy(g[tag + "weight"]).reshape(-1)
        m = (w > 1e-4) & ((w - 1e-4).abs() > 1e-6)
        assert int(m.sum()) >= 50
        assert_close(q["sigma"], g[tag + "sigma"].reshape(-1), f"{tag}sigma", mask=v, elem=FWD_ELEM)
        assert_close(q["rgb"], g[tag + "rgb"].reshape(-1, 3), f"{tag}rgb", mask=m[:, None].expand(-1, 3), elem=FWD_ELEM)
        if which == "dynamic":
            assert_close(q["blending"], g[tag + "blending"].reshape(-1), f"{tag}blending", mask=v, elem=FWD_ELEM)
            assert_close(q["xyz_prime"], g[tag + "xyz_prime"].reshape(-1, 3), f"{tag}xyz_prime", mask=v[:, None].expand(-1, 3),
                         elem=FWD_ELEM)


# ---- 3. tile independence, 4. time modes ----------------------------------------------------------------------------------------
def batch165(spread_times=False):
    """165 valid sample points of ndc_relu (five tiles and a partial one) with their view directions; times per point"""
    c = case("ndc_relu")
    idx = torch.nonzero(c["valid"]).reshape(-1)[:165]
    assert idx.numel() == 165
    t = c["t"][idx]
    if spread_times:   # 12 distinct times, interleaved so that every tile mixes them
        t = (torch.arange(165, device=DEV) % 12).float() * 2 / 11 - 1
    return c, c["pts"][idx].contiguous(), t.contiguous(), c["vd"][idx].contiguous()


@pytest.mark.parametrize("which", ["static", "dynamic"])
def test_a_point_does_not_depend_on_its_tile(which):
    c, pts, t, vd = batch165(spread_times=True)
    field = c["fields"][which]
    full = field.query_points(pts, t, vd, want=OUTS[which])
    perm = torch.randperm(165, generator=torch.Generator().manual_seed(5)).to(DEV)
    shuffled = field.query_points(pts[perm], t[perm], vd[perm], want=OUTS[which])
    for k in OUTS[which]:
        assert same_bits(shuffled[k], full[k][perm]), k
    for M in (1, 31, 32, 33):
        part = field.query_points(pts[:M], t[:M], vd[:M], want=OUTS[which])
        for k in OUTS[which]:
            assert same_bits(part[k], full[k][:M]), (M, k)
    empty = field.query_points(pts[:0], t[:0], vd[:0], want=OUTS[which])
    for k in OUTS[which]:
        assert empty[k].shape == ((0, 3) if k in ("rgb", "xyz_prime") else (0,)) and empty[k].device.type == "cuda", k
    lead = field.query_points(pts[:160].view(5, 32, 3), t[:160].view(5, 32), vd[:160].view(5, 32, 3), want=OUTS[which])
    for k in OUTS[which]:
        assert same_bits(lead[k].reshape(full[k][:160].shape), full[k][:160]), k


def test_one_time_and_a_time_per_point():
    c, pts, t, vd = batch165(spread_times=True)
    dy, st = c["fields"]["dynamic"], c["fields"]["static"]
    shared = dy.query_points(pts, 0.25, vd, want=OUTS["dynamic"])
    filled = dy.query_points(pts, torch.full((165,), 0.25, device=DEV), vd, want=OUTS["dynamic"])
    for k in OUTS["dynamic"]:
        assert same_bits(shared[k], filled[k]), k
    per_point = dy.query_points(pts, t, vd, want=OUTS["dynamic"])
    times = torch.unique(t)
    assert times.numel() == 12
    for tv in times.tolist():
        m = t == tv
        one = dy.query_points(pts[m], tv, vd[m], want=OUTS["dynamic"])
        for k in OUTS["dynamic"]:
            assert same_bits(one[k], per_point[k][m]), (tv, k)
    assert not same_bits(shared["sigma"], per_point["sigma"])   # the time is read
    a, b = st.query_points(pts, None, vd), st.query_points(pts, t, vd)   # the static field does not read it
    for k in OUTS["static"]:
        assert same_bits(a[k], b[k]), k


# ---- 5. view directions -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,which", [("ndc_relu", "dynamic"), ("ndc_relu", "static"), ("contract_relu_te", "static")])
def test_view_directions_are_read_and_used_as_given(name, which):
    """the dynamic head and the two static heads (ndc_relu: MLP_Fea, contract_relu_te: MLP_Fea_TimeEmbedding)"""
    c = case(name)
    field = c["fields"][which]
    assert which == "dynamic" or field.shadingMode == ("MLP_Fea" if name == "ndc_relu" else "MLP_Fea_TimeEmbedding")
    idx = torch.nonzero(c["valid"]).reshape(-1)[:165]
    pts, t, vd = c["pts"][idx].contiguous(), c["t"][idx].contiguous(), c["vd"][idx].contiguous()
    base = field.query_points(pts, t, vd, want=OUTS[which])
    raw = (0.3, -1.7, 2.2)   # not a unit vector
    other = field.query_points(pts, t, raw, want=OUTS[which])
    assert not same_bits(other["rgb"], base["rgb"]) and float((other["rgb"] - base["rgb"]).abs().max()) > 1e-3
    for k in OUTS[which]:
        if k != "rgb":
            assert same_bits(other[k], base[k]), k
    sd, cfg = c["sd"][which]
    vraw = torch.tensor(raw).expand(165, 3)
    ref = point_reference(sd, cfg, pts.cpu(), t.cpu(), vraw, which == "dynamic")
    assert_close(other["rgb"], ref["rgb"], f"{name} {which} rgb, raw view direction", elem=FWD_ELEM)
    unit = point_reference(sd, cfg, pts.cpu(), t.cpu(), vraw / vraw.norm(dim=-1, keepdim=True), which == "dynamic")
    assert float((unit["rgb"] - ref["rgb"]).abs().max()) > 10 * 1e-4 * float(ref["rgb"].abs().max())   # ten times the bound: the check tells them apart
    rows = field.query_points(pts, t, torch.tensor(raw, device=DEV).expand(165, 3), want=("rgb",))   # one vector = its rows
    assert same_bits(rows["rgb"], other["rgb"])


# ---- 6. surface ---------------------------------------------------------------------------------------------------------------
def test_call_surface():
    import rodynrf
    c, pts, t, vd = batch165()
    dy, st = c["fields"]["dynamic"], c["fields"]["static"]
    E = rodynrf.RdrfError
    with pytest.raises(E):
        dy.query_points(pts.reshape(-1))                      # not [..., 3]
    with pytest.raises(E):
        dy.query_points(pts, None, vd)                        # the dynamic field needs a time
    with pytest.raises(E):
        dy.query_points(pts, t[:100], vd)                     # times of another shape
    with pytest.raises(E):
        st.query_points(pts, t[:100], vd)                     # ... refused by the static field too
    with pytest.raises(E):
        dy.query_points(pts, t)                               # rgb wanted, no view directions
    with pytest.raises(E):
        dy.query_points(pts, t, vd[:100])
    with pytest.raises(E):
        st.query_points(pts, None, vd, want=("sigma", "blending"))   # a dynamic output of the static field
    with pytest.raises(E):
        dy.query_points(pts.cpu(), t, vd)
    with pytest.raises(E):
        dy.query_points(pts, t.cpu(), vd)
    with pytest.raises(E):
        dy.query_points(pts, t, vd.cpu())
    full = dy.query_points(pts, t, vd, want=OUTS["dynamic"])
    only = dy.query_points(pts, t, want=("sigma",))           # no appearance phase: no view directions needed
    assert set(only) == {"sigma"} and same_bits(only["sigma"], full["sigma"])
    assert set(rodynrf.query_points(st, pts, viewdirs=vd)) == {"sigma", "rgb"}
    req = pts.clone().requires_grad_(True)                      # no_grad semantics: detached, nothing differentiable
    out = dy.query_points(req, t, vd)
    assert not out["rgb"].requires_grad and same_bits(out["rgb"], full["rgb"])
    for field, which in ((st, "static"), (dy, "dynamic")):     # chunking, with the chunk size lowered
        whole = field.query_points(pts, t, vd, want=OUTS[which])
        chunked = field.query_points(pts, t, vd, want=OUTS[which], _chunk=64)
        parts = [field.query_points(pts[a:a + 64], t[a:a + 64], vd[a:a + 64], want=OUTS[which]) for a in range(0, 165, 64)]
        for k in OUTS[which]:
            assert same_bits(chunked[k], torch.cat([p[k] for p in parts])) and same_bits(chunked[k], whole[k]), k
        shared = field.query_points(pts, 0.25, (0.0, 0.0, 1.0), want=OUTS[which], _chunk=33)   # one time, one direction
        for k in OUTS[which]:
            assert same_bits(shared[k], field.query_points(pts, 0.25, (0.0, 0.0, 1.0), want=OUTS[which])[k]), k


def test_workspace_size_is_what_the_launch_demands():
    """the exact size runs, one byte less is refused (on the device this time: the CPU test sees the refusal only)"""
    import ctypes as C
    L = pkg()
    F = pkg("fields")
    c, pts, t, vd = batch165()
    for which, dyn in (("static", 0), ("dynamic", 1)):
        field = c["fields"][which]
        P, cfg = F.field_structs(field, field._param_list(), "ndc")
        for per_point in (0, 1):
            need = L.lib.rdrf_query_points_ws_bytes(dyn, 165, per_point)
            ws = torch.empty(need, dtype=torch.uint8, device=DEV)
            sigma, rgb = torch.empty(165, device=DEV), torch.empty(165, 3, device=DEV)
            call = lambda nbytes: L.lib.rdrf_query_points(C.byref(P), dyn, C.byref(cfg), L.ptr(pts), 165, L.ptr(t), per_point, L.ptr(vd),
                                                          L.ptr(sigma), L.ptr(rgb), None, None, L.ptr(ws), nbytes, L.stream_of(pts))
            assert call(need - 1) == -3
            assert call(need) == 0
            ref = field.query_points(pts, t if per_point else float(t[0]), vd)
            assert same_bits(sigma, ref["sigma"]) and same_bits(rgb, ref["rgb"])


# ---- 7. meshes ----------------------------------------------------------------------------------------------------------------
def mid_level(field, t):
    alpha, _ = field.getDenseAlpha(LATTICE, times=[0.0 if t is None else t])
    lo, hi = float(alpha.min()), float(alpha.max())
    assert hi > lo
    return 0.5 * (lo + hi)


@pytest.mark.parametrize("which", ["static", "dynamic"])
def test_colored_mesh(which, tmp_path):
    import rodynrf
    field = case("ndc_relu")["fields"][which]
    t = None if which == "static" else 0.25
    level = mid_level(field, t)
    view = (0.0, 0.6, 0.8)
    verts, faces, nrm = rodynrf.field_mesh(field, t, level, LATTICE, normals=True)
    assert verts.shape[0] > 0 and faces.shape[0] > 0
    cv, cf, cn, colors = rodynrf.colored_mesh(field, t, level, LATTICE, view=view, normals=True)
    assert torch.equal(cv, verts) and torch.equal(cf, faces) and torch.equal(cn, nrm)
    assert colors.dtype == torch.uint8 and colors.shape == (verts.shape[0], 3)
    assert torch.equal(colors, rodynrf.vertex_colors(field, verts, t, view))
    rgb = field.query_points(verts, t, view, want=("rgb",))["rgb"]
    assert torch.equal(colors, torch.round(rgb.clamp(0, 1) * 255).to(torch.uint8))
    assert int(colors.max()) > int(colors.min())
    assert not torch.equal(colors, rodynrf.vertex_colors(field, verts, t, (0.0, 0.0, 1.0)))   # the view is read
    three = rodynrf.colored_mesh(field, t, level, LATTICE, view=view)
    assert len(three) == 3 and torch.equal(three[0], verts) and torch.equal(three[2], colors)
    if which == "dynamic":
        with pytest.raises(rodynrf.RdrfError):
            rodynrf.colored_mesh(field, None, level, LATTICE)
    # the PLY carries the colours; a checkpoint gives the same bytes as the live field
    path = str(tmp_path / "mesh.ply")
    out = field.export_mesh(path, t, level, gridSize=LATTICE, normals=True, color_view=view)
    assert len(out) == 4 and torch.equal(out[3], colors)
    back = rodynrf.read_ply(path)
    for key, o in zip(("verts", "faces", "normals", "colors"), (verts, faces, nrm, colors)):
        assert back[key].tobytes() == o.cpu().numpy().tobytes(), key
    with pytest.raises(rodynrf.RdrfError):
        field.export_mesh(path, t, level, gridSize=LATTICE, color_view=view, colors=colors)   # colours come through color_view only
    ckpt = str(tmp_path / "field.th")
    field.save(torch.eye(3, 4)[None].repeat(12, 1, 1), torch.tensor(1.0), ckpt)
    path2 = str(tmp_path / "from_ckpt.ply")
    rodynrf.export_mesh(ckpt, path2, t, level, gridSize=LATTICE, normals=True, device=DEV, color_view=view)
    assert open(path2, "rb").read() == open(path, "rb").read()
    # world space moves the vertices and keeps the colours
    H, W, focal = 27.0, 48.0, 41.5
    wv, wf, wc = rodynrf.colored_mesh(field, t, level, LATTICE, view=view, space="world", H=H, W=W, focal=focal)
    fv, ff = rodynrf.field_mesh(field, t, level, LATTICE, space="world", H=H, W=W, focal=focal)
    assert torch.equal(wv, fv) and torch.equal(wf, ff) and torch.equal(wc, colors)


# ---- 8. deterministic twin ------------------------------------------------------------------------------------------------------
def det_case():
    """what both libraries run (tests/_det_child.py case)"""
    c, pts, t, vd = batch165(spread_times=True)
    out = {}
    for which, field in c["fields"].items():
        for mode, tt in (("per_point", t), ("shared", 0.25)):
            for k, v in field.query_points(pts, tt, vd, want=OUTS[which]).items():
                out[f"{which}.{mode}.{k}"] = v.cpu()
    return out


def test_deterministic_library_gives_the_same_bits(tmp_path):
    ours = det_case()
    assert len(ours) == 12
    assert_same_dict(run_twin(tmp_path, [CHILD, "case", "test_gpu_point_query"], det=True), ours)
