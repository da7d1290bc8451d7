"""The masked render (render_rays(..., alpha_masks=...), rdrf_render_masked_fwd) against the composition that defines it:

    xyz, z, valid = sampleXYZ(...); valid_s = apply_alpha_mask(valid, xyz, ts, mask_s); valid_d = ... mask_d;
    static forward with valid_s, dynamic forward with valid_d, raw2outputs

run in the same test; every RenderMaps field with torch.equal.  The density kernels of the masked render run over lists of
kept samples in 32-entry tiles, so the shapes and masks below put list lengths at 0, inside one tile and past a tile without
filling the last one, tiles that span several rays and tiles that straddle a ray's end."""
import functools

import pytest
import torch

import _util
from _twin import CHILD, assert_same_dict, run_twin
from _util import pkg

pytestmark = pytest.mark.gpu

DEV = "cuda"
CASES = ("ndc_relu", "contract_softplus_te", "world")
SHAPES = ((1, 13), (7, 13), (5, 33), (64, 115), (257, 31))
VOL = (7, 6, 5, 3)   # (G2, G1, G0, T) of every mask volume
SLOTS = dict(rgb=0, depth=1, acc=2, rgb_s=4, depth_s=5, acc_s=6, rgb_d=8, depth_d=9, acc_d=10, blending=12)
PARTIAL = ("slab", "random", "random2", "time0", "cell")
# (static mask kind, dynamic mask kind): the five volumes on both fields, one field masked only, two different masks
PAIRS = (("ones", "ones"), ("zeros", "zeros"), ("slab", "slab"), ("random", "random"), ("time0", "time0"), ("random", None),
         (None, "random"), ("slab", "random2"))
# the whole parametrisation (the kept-count coverage test walks it)
PARAMS = [(c, n, s, ("random", "random2")) for c in CASES for n, s in SHAPES]
PARAMS += [(c, 64, 115, p) for c in CASES for p in PAIRS]
PARAMS += [(c, n, 13, ("cell", "cell")) for c in CASES for n in (1, 7)]
IDS = [f"{c}-{n}x{s}-{p[0]}-{p[1]}" for c, n, s, p in PARAMS]


@functools.lru_cache(maxsize=None)
def fields(case):
    """(static field, dynamic field, ray_type) of a golden case's small grid; "world": the fields of tests/test_gpu_world_rays.py"""
    if case == "world":
        import test_gpu_world_rays as W
        st, dy = W.fields("a")
        return st, dy, "world"
    from _gpu_util import fields_from_case
    _, st, dy, _ = fields_from_case(case, DEV)
    return st, dy, case.split("_")[0]


def make_rays(case, N):
    """N rays that cross the field's box and their times, spread over [-1, 1]"""
    from _gpu_util import make_rays as mk
    st, dy, rt = fields(case)
    ts = torch.linspace(-1.0, 1.0, N) if N > 1 else torch.tensor([-1.0])
    if rt != "world":
        rays, _ = mk(N, 11 + N, rt)
        return rays.to(DEV), ts.to(DEV)
    g = torch.Generator().manual_seed(11 + N)
    lo, hi = dy.aabb.detach().cpu()
    c, half = (lo + hi) / 2, (hi - lo) / 2
    o = c + torch.stack([(torch.rand(N, generator=g) - 0.5) * half[0], (torch.rand(N, generator=g) - 0.5) * half[1],
                         torch.full((N,), -3.0 * float(half[2]))], -1)
    d = torch.stack([torch.randn(N, generator=g) * 0.08, torch.randn(N, generator=g) * 0.08, torch.ones(N)], -1)
    d = d / d.norm(dim=-1, keepdim=True)
    return torch.cat([o, d], -1).to(DEV), ts.to(DEV)


def sub_box(field):
    """a strict sub-box of the field's aabb: the mask's zero padding outside it is exercised"""
    lo, hi = field.aabb.detach().cpu()
    size = hi - lo
    return torch.stack([lo + 0.15 * size, hi - 0.10 * size])


def make_mask(kind, field, xyz=None, valid=None, box=None):
    """the mask volumes of the issue: all ones, all zeros, a depth slab, a seeded random volume (~30 % occupied), slice 0 only,
    and one occupied cell on the path of ray 0"""
    rodynrf = _util.rodynrf()
    if kind is None:
        return None
    G2, G1, G0, T = VOL
    box = sub_box(field) if box is None else box
    vol = torch.zeros(VOL)
    if kind == "ones":
        vol[:] = 1
    elif kind == "slab":
        vol[2:4] = 1
    elif kind in ("random", "random2"):
        g = torch.Generator().manual_seed(5 if kind == "random" else 6)
        vol = (torch.rand(VOL, generator=g) < 0.3).float()
    elif kind == "time0":
        vol[..., 0] = 1
    elif kind == "cell":   # the voxel nearest to a sample of ray 0 inside the mask's box, every slice
        p = xyz[0].detach().cpu()
        inside = ((p > box[0]) & (p < box[1])).all(-1) & valid[0].cpu().bool()
        assert bool(inside.any()), "ray 0 misses the mask's box"
        q = p[inside][int(inside.sum()) // 2]
        f = (q - box[0]) / (box[1] - box[0]) * torch.tensor([G0 - 1.0, G1 - 1.0, G2 - 1.0])
        ix, iy, iz = (int(v) for v in f.round())
        vol[iz, iy, ix, :] = 1
    elif kind != "zeros":
        raise ValueError(kind)
    return rodynrf.AlphaGridMask(DEV, box, vol, T)


def composed(case, rays, ts, S, masks):
    """the defining composition -> (the 13 outputs of raw2outputs, valid, valid_s, valid_d)"""
    rodynrf = _util.rodynrf()
    st, dy, rt = fields(case)
    with torch.no_grad():
        xyz, z, valid = rodynrf.sampleXYZ(dy, rays, S, ray_type=rt, is_train=False)
        vs = rodynrf.apply_alpha_mask(valid, xyz, ts, masks[0])
        vd = rodynrf.apply_alpha_mask(valid, xyz, ts, masks[1])
        o_s = st(rays, ts, None, xyz, z, vs, is_train=False, ray_type=rt, N_samples=S)
        o_d = dy(rays, ts, None, xyz, z, vd, is_train=False, ray_type=rt, N_samples=S)
        outs = rodynrf.raw2outputs(o_s[6], o_s[7], o_d[6], o_d[7], o_d[9], o_d[2], o_d[8], rays, is_train=False, ray_type=rt)
    return outs, valid, vs, vd


def masks_for(case, N, S, pair):
    rodynrf = _util.rodynrf()
    st, dy, rt = fields(case)
    rays, ts = make_rays(case, N)
    xyz = valid = None
    if "cell" in pair:
        with torch.no_grad():
            xyz, _, valid = rodynrf.sampleXYZ(dy, rays, S, ray_type=rt, is_train=False)
    return rays, ts, (make_mask(pair[0], st, xyz, valid), make_mask(pair[1], dy, xyz, valid))


def same_maps(m, ref, what):
    for n, i in SLOTS.items():
        got = getattr(m, n)
        assert got is not None and torch.equal(got.reshape(ref[i].shape), ref[i]), f"{what}: {n}"


@functools.lru_cache(maxsize=None)
def run_case(case, N, S, pair):
    """one masked render checked against the composition -> (kept_s, kept_d, valid count, partial flags)"""
    rodynrf = _util.rodynrf()
    st, dy, rt = fields(case)
    rays, ts, masks = masks_for(case, N, S, pair)
    ref, valid, vs, vd = composed(case, rays, ts, S, masks)
    kept = torch.full((2,), -1, dtype=torch.int64, device=DEV)
    m = rodynrf.render_rays(st, dy, rays, ts, S, ray_type=rt, maps=True, alpha_masks=masks, kept=kept)
    what = f"{case} {N}x{S} {pair}"
    same_maps(m, ref, what)
    k = [int(v) for v in kept.cpu()]
    nv = int(valid.sum())
    print(f"{what}: kept {k} of {nv} valid samples ({N * S} samples)")
    assert k == [int(vs.sum()), int(vd.sum())], (what, k)
    # the pair form of the outputs, and a second call: the same bits
    rgb, depth = rodynrf.render_rays(st, dy, rays, ts, S, ray_type=rt, alpha_masks=masks)
    assert torch.equal(rgb, ref[0]) and torch.equal(depth, ref[1]), what
    same_maps(rodynrf.render_rays(st, dy, rays, ts, S, ray_type=rt, maps=True, alpha_masks=masks), ref, what + " (again)")
    partial = [p in PARTIAL for p in pair]
    if any(partial):
        for f in (0, 1):
            if partial[f]:
                assert 0 < k[f] < nv, (what, f, k, nv)
            elif pair[f] is None:
                assert k[f] == nv, (what, f, k, nv)
        plain = rodynrf.render_rays(st, dy, rays, ts, S, ray_type=rt, maps=True)
        assert not torch.equal(plain.rgb, m.rgb), f"{what}: the masks change no ray's colour"
    return k[0], k[1], nv


@pytest.mark.parametrize("case,N,S,pair", PARAMS, ids=IDS)
def test_masked_render_equals_the_composition(case, N, S, pair):
    run_case(case, N, S, pair)


def test_kept_counts_cover_the_tile_edges():
    """across the parametrisation a kept list is empty, shorter than one 32-entry tile, and longer than one without being
    whole tiles: no case has silently degenerated"""
    counts = []
    for p in PARAMS:
        ks, kd, _ = run_case(*p)
        counts += [ks, kd]
    assert any(c == 0 for c in counts), sorted(set(counts))
    assert any(0 < c < 32 for c in counts), sorted(set(counts))
    assert any(c > 32 and c % 32 != 0 for c in counts), sorted(set(counts))


@pytest.mark.parametrize("case", CASES)
def test_trivial_masks(case):
    """all-ones masks over a box that holds the field's give the bits of the unmasked render; all-zero masks the composition's
    (every sample dropped)"""
    rodynrf = _util.rodynrf()
    st, dy, rt = fields(case)
    N, S = 64, 115
    rays, ts = make_rays(case, N)
    lo, hi = dy.aabb.detach().cpu()
    big = torch.stack([lo - 0.05 * (hi - lo), hi + 0.05 * (hi - lo)])
    ones = (make_mask("ones", st, box=big), make_mask("ones", dy, box=big))
    kept = torch.zeros(2, dtype=torch.int64, device=DEV)
    m = rodynrf.render_rays(st, dy, rays, ts, S, ray_type=rt, maps=True, alpha_masks=ones, kept=kept)
    plain = rodynrf.render_rays(st, dy, rays, ts, S, ray_type=rt, maps=True)
    for n in SLOTS:
        assert torch.equal(getattr(m, n), getattr(plain, n)), f"{case}: all-ones masks change {n}"
    ref, valid, _, _ = composed(case, rays, ts, S, ones)
    same_maps(m, ref, f"{case} all ones")
    assert [int(v) for v in kept.cpu()] == [int(valid.sum())] * 2 and int(valid.sum()) > 0
    zeros = (make_mask("zeros", st), make_mask("zeros", dy))
    m0 = rodynrf.render_rays(st, dy, rays, ts, S, ray_type=rt, maps=True, alpha_masks=zeros, kept=kept)
    same_maps(m0, composed(case, rays, ts, S, zeros)[0], f"{case} all zeros")
    assert [int(v) for v in kept.cpu()] == [0, 0]
    assert float(m0.acc.abs().max()) == 0.0


@pytest.mark.parametrize("case", CASES)
def test_poisoned_workspace_changes_no_bit(case):
    """nothing downstream of the keep pass depends on what the workspace held before the call"""
    from test_gpu_poisoned_scratch import scratch_fill
    rodynrf = _util.rodynrf()
    st, dy, rt = fields(case)
    N, S, pair = 64, 115, ("slab", "random2")
    rays, ts, masks = masks_for(case, N, S, pair)
    ref = composed(case, rays, ts, S, masks)[0]
    with scratch_fill(0xFF) as seen:
        m = rodynrf.render_rays(st, dy, rays, ts, S, ray_type=rt, maps=True, alpha_masks=masks)
    assert seen["workspace"] >= 1, seen
    for n in SLOTS:
        assert bool(torch.isfinite(getattr(m, n)).all()), n
    same_maps(m, ref, f"{case} on a NaN-filled workspace")


def view_case():
    """a 9 x 7 view of the ndc case with two different masks: whole image, in chunks of 20 rays"""
    rodynrf = _util.rodynrf()
    st, dy, rt = fields("ndc_relu")
    masks = (make_mask("slab", st), make_mask("random2", dy))
    c2w = torch.tensor([[1.0, 0.0, 0.0, 0.05], [0.0, 1.0, 0.0, -0.02], [0.0, 0.0, 1.0, 0.0]])
    whole = rodynrf.render_view(st, dy, c2w, 8.0, 7, 9, 0.3, 33, ray_type=rt, maps=True, alpha_masks=masks)
    parts = rodynrf.render_view(st, dy, c2w, 8.0, 7, 9, 0.3, 33, ray_type=rt, maps=True, chunk=20, alpha_masks=masks)
    return whole, parts


def det_case():
    """what both libraries compute (tests/_det_child.py case): the maps of two masked renders"""
    rodynrf = _util.rodynrf()
    out = {}
    for case in ("ndc_relu", "contract_softplus_te"):
        st, dy, rt = fields(case)
        rays, ts, masks = masks_for(case, 64, 115, ("slab", "random2"))
        kept = torch.zeros(2, dtype=torch.int64, device=DEV)
        m = rodynrf.render_rays(st, dy, rays, ts, 115, ray_type=rt, maps=True, alpha_masks=masks, kept=kept)
        out.update({f"{case}.{n}": getattr(m, n) for n in SLOTS})
        out[f"{case}.kept"] = kept
    return out


def test_chunked_image_equals_the_whole_image():
    whole, parts = view_case()
    for n in SLOTS:
        assert torch.equal(getattr(whole, n), getattr(parts, n)), n


def test_deterministic_library_gives_the_same_bits(tmp_path):
    """librodynrf_det.so exports the entry points and runs the same path: the maps and the kept counts of the default build"""
    ours = det_case()
    assert_same_dict(run_twin(tmp_path, [CHILD, "case", "test_gpu_masked_render"], det=True), ours)


def test_render_view_with_the_fields_own_masks():
    """updateAlphaMask on both fields of a small case, then render_view(alpha_masks=True): the composition with the fields'
    alphaMask, clamped as render_view clamps"""
    from _gpu_util import fields_from_case
    rodynrf = _util.rodynrf()
    _, st, dy, _ = fields_from_case("ndc_relu", DEV)   # fresh fields: the masks stay out of the shared ones
    lat = (12, 13, 8)
    for f in (st, dy):
        alpha, _ = f.getDenseAlpha(lat)
        f.alphaMask_thres = float(alpha.flatten().kthvalue(int(alpha.numel() * 0.9)).values)   # ~10 % of the lattice above it
        f.updateAlphaMask(lat)
        assert 0 < f.alphaMask_stats["occupied"] < f.alphaMask_stats["total"]
    with pytest.raises(ValueError):
        rodynrf.render_rays(fields("ndc_relu")[0], fields("ndc_relu")[1], *make_rays("ndc_relu", 7), 13, alpha_masks=True)
    H, W, focal, t, S = 7, 9, 8.0, -0.4, 33
    c2w = torch.tensor([[1.0, 0.0, 0.0, 0.05], [0.0, 1.0, 0.0, -0.02], [0.0, 0.0, 1.0, 0.0]])
    rays = rodynrf.camera_rays(c2w.to(DEV).reshape(1, 3, 4), focal, H, W, ndc=True, near=1.0)
    ts = torch.full((H * W,), t, device=DEV)
    with torch.no_grad():
        xyz, z, valid = rodynrf.sampleXYZ(dy, rays, S, ray_type="ndc", is_train=False)
        vs = rodynrf.apply_alpha_mask(valid, xyz, ts, st.alphaMask)
        vd = rodynrf.apply_alpha_mask(valid, xyz, ts, dy.alphaMask)
        o_s = st(rays, ts, None, xyz, z, vs, is_train=False, ray_type="ndc", N_samples=S)
        o_d = dy(rays, ts, None, xyz, z, vd, is_train=False, ray_type="ndc", N_samples=S)
        ref = list(rodynrf.raw2outputs(o_s[6], o_s[7], o_d[6], o_d[7], o_d[9], o_d[2], o_d[8], rays, is_train=False, ray_type="ndc"))
    assert 0 < int(vs.sum()) < int(valid.sum()) and 0 < int(vd.sum()) < int(valid.sum())
    for i in (0, 4, 8, 12):
        ref[i] = ref[i].clamp(0.0, 1.0)
    m = rodynrf.render_view(st, dy, c2w, focal, H, W, t, S, ray_type="ndc", maps=True, alpha_masks=True)
    same_maps(m, ref, "render_view(alpha_masks=True)")
    rgb, depth = rodynrf.render_view(st, dy, c2w, focal, H, W, t, S, ray_type="ndc", maps=False, alpha_masks=True)
    assert torch.equal(rgb.reshape(-1, 3), ref[0]) and torch.equal(depth.reshape(-1), ref[1])
    frames = list(rodynrf.render_path(st, dy, [c2w], focal, H, W, change_time=t, N_samples=S, ray_type="ndc", alpha_masks=True))
    same_maps(frames[0], ref, "render_path(alpha_masks=True)")


def test_out_of_scope_combinations_raise():
    rodynrf = _util.rodynrf()
    st, dy, rt = fields("ndc_relu")
    rays, ts, masks = masks_for("ndc_relu", 7, 13, ("slab", "slab"))
    eye = torch.eye(4)[:3]
    with pytest.raises(NotImplementedError):
        rodynrf.render_rays(st, dy, rays, ts, 13, ray_type=rt, mode="fused", alpha_masks=masks)
    with pytest.raises(NotImplementedError):
        rodynrf.render_rays(st, dy, rays, ts, 13, ray_type=rt, alpha_masks=masks,
                            motion=dict(H=1, W=7, focal=10.0, c2w_f=eye, c2w_b=eye))
    R = pkg("renderer")
    with pytest.raises(NotImplementedError):
        R.render_chunks(st, dy, rays, ts, 4, 13, ray_type=rt, alpha_masks=masks)
    with pytest.raises(ValueError):
        rodynrf.render_rays(st, dy, rays, ts, 13, ray_type=rt, alpha_masks=(None, None))
