"""The per-field ray scan on arrays of its own (rdrf_selftest_ray_scan: k_ray_scan 32 wide, k_static_scan 64 wide;
rdrf_selftest_ray_scan_bwd: k_ray_scan_bwd, k_static_density_bwd -- the kernels and the launch geometry of the entry points)
against the float64 reference of tests/_scan_prim.py, on the regimes whole fields with random weights never reach: opaque samples
on both sides of every 32- and 64-sample tile edge, runs of them (T down to 1e-40), empty rays, rays with no or few valid samples,
raw values around the activations' kinks, S = 4096 (every carry slot), every cotangent alone.

Shapes: N = 35 rays (width 32: two 16-ray workgroups and a partial one, one half-wave without a ray; width 64: no multiple of the
4 waves of a workgroup), S in {1, 2, 31, 32, 33, 63, 64, 65, 129, 257}, N = 3 at S = 4096; ndc, contract and world rays, relu and
softplus, distance_scale 25 and 1.

Bound of every comparison (derived in tests/_scan_prim.py, not tuned):  max|err| <= 1e-4 max|ref| + c 2^-23 max(condition scale),
c = the compositor's 6 S + S / 64 + 32, + 5 S for forming ds from z and |d|, + 5 S for softplus on the backward side, + S / 32 -
S / 64 at width 32.  g_z and g_rays are accumulated into small integers; their pre-fill joins the reference and the condition
scale.  The walls of `wall`, `double_wall` and `invalid` sit on both sides of every 32-sample edge over the N = 35 rays
(_scan_prim.wall_position); at S = 4096 the N = 3 case holds samples 0, 31 and 32 and a sweep of 255 rays holds every edge.

dists.  Both sides take dz = fl(z[j+1] - z[j]), the same fp32 subtraction of the same operands: one value, no error between them.
World rays: weight_round forms fl(fl(dz * 1.0f) * scale) = fl(dz * scale): bit-equal to that fp32 product.  ndc / contract rays,
against the exact dz |d| scale, relative errors in units of u = 2^-24, line by line:
  ray_norm   x x, y y, z z            one rounding each                                    1 u on every term
             (x x + y y) + z z        two sums, the longest path through both              3 u on the sum of squares  (fma: less)
             sqrtf                    halves the relative error, rounds once               1.5 u + 1 u = 2.5 u on |d|
  weight_round  dz * nrm              one rounding                                         3.5 u
             ... * distance_scale     one rounding                                         4.5 u
4.5 u = 2.25 ulp: the test allows 3 ulp.
The compaction is checked exactly, against the kernel's own stored weights.  profiles/scan_margins.txt holds the ratios of one run."""

import numpy as np
import pytest
import torch

import _scan_prim as Q
from _twin import CHILD, run_twin, tools_lib
from _util import pkg, record_margin

pytestmark = pytest.mark.gpu

N = Q.N_RAYS
GUARD = 64
IPOISON = -777
CNT0 = 5                                           # the counter's pre-fill: it is added to, not set
COMBOS = (("relu", "ndc", 25.0), ("softplus", "contract", 1.0), ("softplus", "world", 25.0), ("relu", "world", 1.0))
RT = {"ndc": 0, "contract": 1, "world": 2}
ACT = {"relu": 0, "softplus": 1}


class Guarded:
    """a device array between two poisoned guard bands"""

    def __init__(self, shape, dtype=torch.float32, fill=None):
        n = 1
        for s in shape:
            n *= s
        self.poison = float("nan") if dtype.is_floating_point else IPOISON
        self.flat = torch.full((n + 2 * GUARD,), self.poison, dtype=dtype, device="cuda")
        self.t = self.flat[GUARD:GUARD + n].view(shape)
        if fill is not None:
            self.t.copy_(fill)

    def guards_intact(self):
        g = torch.cat([self.flat[:GUARD], self.flat[-GUARD:]]).cpu()
        return bool(torch.isnan(g).all()) if g.is_floating_point() else bool((g == IPOISON).all())


def run_fwd(width, x, rt, scale, thres, rgb=True):
    """-> weight, dists [N,S], list (whole buffer), counter, rgb or None, all on the CPU"""
    L = pkg()
    n, S = x["z"].shape
    rays, z, sigma = x["rays"].cuda(), x["z"].cuda(), x["sigma"].cuda()
    w, d = Guarded((n, S)), Guarded((n, S))
    lst = Guarded((n * S + CNT0,), torch.int32)
    cnt = torch.full((64,), CNT0, dtype=torch.int32, device="cuda")
    c = Guarded((n, S, 3)) if rgb else None
    L.check(L.lib.rdrf_selftest_ray_scan(width, L.ptr(rays), L.ptr(z), L.ptr(sigma), n, S, RT[rt], scale, thres, L.ptr(w.t),
                                         L.ptr(d.t), L.ptr(lst.t), L.ptr(cnt), L.ptr(c.t if rgb else None), L.stream_of(z)),
            "rdrf_selftest_ray_scan")
    torch.cuda.synchronize()
    for g, name in ((w, "weight"), (d, "dists"), (lst, "list"), (c, "rgb")):
        assert g is None or g.guards_intact(), f"the guard bands of {name} were written"
    assert bool((cnt[1:] == CNT0).all()), "ints behind the counter were written"
    return w.t.cpu(), d.t.cpu(), lst.t.cpu(), int(cnt[0]), (c.t.cpu() if rgb else None)


def _prefill(n, S):
    j = torch.arange(S)[None, :] + torch.arange(n)[:, None]
    return (j % 4 - 1).float(), ((torch.arange(6)[None, :] + torch.arange(n)[:, None]) % 3 + 1).float()


def run_bwd(width, x, act, rt, scale, cot, want_z=True, want_rays=True, rows=None):
    """-> out ([N,S] gsig or [N,Sp] gf rows, poison kept), g_z, g_rays (None where not asked) on the CPU.  rows: run these rays
    alone, pre-filled as the full run pre-fills them"""
    L = pkg()
    n, S = x["z"].shape
    pz, pr = _prefill(n, S)
    sel = slice(None) if rows is None else rows
    rays, z, valid = x["rays"][sel].contiguous().cuda(), x["z"][sel].contiguous().cuda(), x["valid"][sel].contiguous().cuda()
    raw = x["raw"][sel].contiguous()
    m = z.shape[0]
    if width == 32:   # slot 0 of [N][S][2]: the density head; slot 1 (blending) is not the scan's to read
        raw = torch.stack([raw, torch.full_like(raw, float("nan"))], -1).contiguous()
    raw = raw.cuda()
    g = [None if cot[k] is None else cot[k][sel].contiguous().cuda() for k in ("w", "s", "d")]
    Sp = S if width == 32 else ((S + 31) // 32) * 32
    out = Guarded((m, Sp))
    gz = Guarded((m, S), fill=pz[sel].cuda()) if want_z else None
    gr = Guarded((m, 6), fill=pr[sel].cuda()) if want_rays else None
    L.check(L.lib.rdrf_selftest_ray_scan_bwd(width, L.ptr(rays), L.ptr(z), L.ptr(valid), L.ptr(raw), m, S, ACT[act], Q.SHIFT, scale,
                                             RT[rt], L.ptr(g[0]), L.ptr(g[1]), L.ptr(g[2]), L.ptr(out.t),
                                             L.ptr(gz.t if want_z else None), L.ptr(gr.t if want_rays else None), L.stream_of(z)),
            "rdrf_selftest_ray_scan_bwd")
    torch.cuda.synchronize()
    for b, name in ((out, "out"), (gz, "g_z"), (gr, "g_rays")):
        assert b is None or b.guards_intact(), f"the guard bands of {name} were written"
    return out.t.cpu(), (gz.t.cpu() if want_z else None), (gr.t.cpu() if want_rays else None)


def _check(got, ref, cond, c, tag, key):
    assert bool(torch.isfinite(got).all()), f"{tag}: NaN / Inf"
    ratio = Q.error_ratio(got, ref, cond, c)
    print(f"{key} | {tag}: {ratio:.4f}")
    record_margin(f"{key} | {tag}", ratio)
    assert ratio <= 1.0, f"{key} | {tag}: max|err| is {ratio:.3f} x (1e-4 max|ref| + c 2^-23 max cond)"


def _check_structure(w, lst, cnt, thres, S, tag):
    """counter, list and its poison against the kernel's own stored weights"""
    want = torch.nonzero(w.reshape(-1) > thres).reshape(-1)
    assert cnt == CNT0 + want.numel(), f"{tag}: counter {cnt}, {want.numel()} weights above the threshold (pre-fill {CNT0})"
    got = lst[CNT0:cnt].long()
    assert bool((lst[:CNT0] == IPOISON).all()) and bool((lst[cnt:] == IPOISON).all()), f"{tag}: list outside [pre-fill, counter) written"
    assert torch.equal(torch.sort(got).values, want), f"{tag}: list is not the set of the weights above the threshold (or has duplicates)"
    order = torch.sort(got // S, stable=True).indices
    assert torch.equal(got[order], want), f"{tag}: a ray's entries are not ascending"


def _check_dists(d, x, rt, scale, tag):
    z = x["z"]
    dz = torch.cat([z[:, 1:] - z[:, :-1], torch.zeros_like(z[:, :1])], -1)      # fp32, one rounding, as the kernel's
    if rt == "world":
        assert torch.equal(d, (dz * 1.0) * torch.tensor(scale, dtype=torch.float32)), f"{tag}: dists differ from the fp32 product"
    else:
        ref = dz.double() * x["rays"][:, 3:6].double().norm(dim=-1, keepdim=True) * scale
        assert bool(((d.double() - ref).abs() <= 3 * Q.EPS32 * ref.abs()).all()), f"{tag}: dists off by more than 3 ulp"


def _check_bwd(width, r, act, rt, scale, out, gz, gr, tag, key):
    n, S = r["x"]["z"].shape
    c = Q.c_ops(S, width, act == "softplus")
    pz, pr = _prefill(n, S)
    name = "gsig" if width == 32 else "gf"
    if width == 64:
        assert bool(torch.isnan(out[:, S:]).all()), f"{tag}: the padding columns of gf_rows were written"
    _check(out[:, :S], r["grads"][name], r["gcond"][name], c, tag, f"w{width} {key} {name}")
    if gz is not None:
        _check(gz, pz.double() + r["grads"]["g_z"], pz.abs().double() + r["gcond"]["g_z"], c, tag, f"w{width} {key} g_z")
    if gr is not None:
        untouched = slice(0, 6) if rt == "world" else slice(0, 3)
        assert torch.equal(gr[:, untouched], pr[:, untouched]), f"{tag}: g_rays written where no gradient flows"
        _check(gr, pr.double() + r["grads"]["g_rays"], pr.abs().double() + r["gcond"]["g_rays"], c, tag, f"w{width} {key} g_rays")


@pytest.mark.parametrize("regime", Q.REGIMES)
@pytest.mark.parametrize("width", [32, 64])
def test_forward_matches_float64_and_compacts_exactly(width, regime):
    for S in Q.SIZES:
        for rt, scale in (("ndc", 25.0), ("contract", 1.0), ("world", 25.0), ("world", 1.0)):
            r = Q.reference(regime, N, S, "relu", rt, scale)
            tag = f"{regime} S={S} {rt} scale={scale:g}"
            for thres in ((1e-4, -1.0, 1e9) if rt in ("ndc", "world") else (1e-4,)):
                w, d, lst, cnt, rgb = run_fwd(width, r["x"], rt, scale, thres)
                _check_structure(w, lst, cnt, thres, S, f"{tag} thres={thres:g}")
                assert bool((rgb == 0).all()), f"{tag}: rgb is not all zero"
                if thres == -1.0:
                    assert cnt == CNT0 + N * S
                if thres == 1e9:
                    assert cnt == CNT0
                if thres == 1e-4:
                    _check(w, r["fwd"]["w"], r["fwd"]["wcond"], Q.c_ops(S, width), tag, f"w{width} {regime} weight")
                    _check_dists(d, r["x"], rt, scale, tag)
                    if regime == "empty":
                        assert bool((r["x"]["sigma"] == 0).all()) and bool((w == 0).all()), f"{tag}: sigma == 0 must give weight == 0.0"
                else:
                    assert torch.equal(w, w0) and torch.equal(d, d0), f"{tag}: weight / dists depend on the threshold"
                w0, d0 = w, d


@pytest.mark.parametrize("width", [32, 64])
def test_forward_accepts_a_null_rgb(width):
    """rgb = NULL: no colour is zeroed and nothing else changes (ndc rays at scale 25, S = 2 and 65)"""
    for regime, S in (("mixed", 2), ("wall", 65)):
        x = Q.generate(regime, N, S, "relu", "ndc", 25.0)
        w1, d1, lst1, cnt1, none = run_fwd(width, x, "ndc", 25.0, 1e-4, rgb=False)
        w2, d2, _, cnt2, rgb = run_fwd(width, x, "ndc", 25.0, 1e-4)
        assert none is None and bool((rgb == 0).all())
        assert torch.equal(w1, w2) and torch.equal(d1, d2) and cnt1 == cnt2
        _check_structure(w1, lst1, cnt1, 1e-4, S, f"{regime} S={S} rgb=NULL")


@pytest.mark.parametrize("width", [32, 64])
def test_forward_behind_one_opaque_sample(width):
    """sigma ds >= 20 at sample k: alpha rounds to 1.0, p is 1e-10, and every weight behind k is at most 1e-10 (1 + c 2^-23)"""
    for S in (2, 33, 65, 257):
        for rt, scale in (("ndc", 25.0), ("world", 1.0)):
            x = Q.generate("thin", N, S, "relu", rt, scale)
            ks = [Q.wall_position(n, S) for n in range(N)]
            for n, k in enumerate(ks):
                x["sigma"][n, k] = Q.opaque_sigma(x, n, k, rt, scale)
            w, d, _, _, _ = run_fwd(width, x, rt, scale, 1e-4)
            lim = 1e-10 * (1.0 + Q.c_ops(S, width) * Q.EPS32)
            for n, k in enumerate(ks):
                assert float(x["sigma"][n, k]) * float(d[n, k]) >= 20.0
                assert float(w[n, k + 1:].abs().max()) <= lim, (S, rt, n, k, float(w[n, k + 1:].abs().max()))
                assert float(w[n, k]) > 0.1


@pytest.mark.parametrize("regime", Q.REGIMES)
@pytest.mark.parametrize("width", [32, 64])
def test_backward_matches_float64(width, regime):
    """all three cotangents; gsig / gf_rows, g_z and g_rays (accumulated into small integers), the padding and the untouched columns"""
    for S in Q.SIZES:
        for act, rt, scale in COMBOS:
            r = Q.reference(regime, N, S, act, rt, scale, ("w", "s", "d"))
            out, gz, gr = run_bwd(width, r["x"], act, rt, scale, r["cot"])
            _check_bwd(width, r, act, rt, scale, out, gz, gr, f"{regime} S={S} {act} {rt} scale={scale:g}", regime)


@pytest.mark.parametrize("cot_set", Q.COT_SETS, ids=lambda s: "+".join(s))
@pytest.mark.parametrize("width", [32, 64])
def test_backward_every_cotangent_set_and_null_output(width, cot_set):
    """each cotangent alone, each pair, all three; with g_z, g_rays or both null"""
    for regime, S, act, rt, scale in (("wall", 65, "relu", "ndc", 25.0), ("mixed", 129, "softplus", "contract", 1.0),
                                      ("invalid", 33, "softplus", "ndc", 25.0), ("act_edges", 64, "relu", "world", 25.0),
                                      ("double_wall", 257, "relu", "contract", 25.0), ("thin", 1, "softplus", "ndc", 1.0)):
        r = Q.reference(regime, N, S, act, rt, scale, cot_set)
        tag = f"{regime} S={S} {act} {rt} cot={'+'.join(cot_set)}"
        full = run_bwd(width, r["x"], act, rt, scale, r["cot"])
        _check_bwd(width, r, act, rt, scale, *full, tag, f"{regime} cot")
        for want_z, want_rays in ((False, True), (True, False), (False, False)):
            out, gz, gr = run_bwd(width, r["x"], act, rt, scale, r["cot"], want_z, want_rays)
            _check_bwd(width, r, act, rt, scale, out, gz, gr, f"{tag} g_z={int(want_z)} g_rays={int(want_rays)}", f"{regime} cot")
            # a null output changes nothing of the others: same group, same order
            assert torch.equal(out[:, :S], full[0][:, :S])
            assert gz is None or torch.equal(gz, full[1])
            assert gr is None or torch.equal(gr, full[2])


@pytest.mark.parametrize("regime", ["wall", "mixed"])
@pytest.mark.parametrize("width", [32, 64])
def test_4096_samples_use_every_carry_slot(width, regime):
    S, n = Q.S_MAX, 3
    act, rt, scale = ("relu", "ndc", 25.0) if regime == "wall" else ("softplus", "contract", 1.0)
    r = Q.reference(regime, n, S, act, rt, scale, ("w", "s", "d"))
    tag = f"{regime} S={S} {act} {rt}"
    w, d, lst, cnt, rgb = run_fwd(width, r["x"], rt, scale, 1e-4)
    _check(w, r["fwd"]["w"], r["fwd"]["wcond"], Q.c_ops(S, width), tag, f"w{width} {regime} weight")
    _check_structure(w, lst, cnt, 1e-4, S, tag)
    _check_dists(d, r["x"], rt, scale, tag)
    assert bool((rgb == 0).all())
    out, gz, gr = run_bwd(width, r["x"], act, rt, scale, r["cot"])
    _check_bwd(width, r, act, rt, scale, out, gz, gr, tag, regime)


@pytest.mark.parametrize("width", [32, 64])
def test_4096_samples_with_a_wall_on_each_side_of_every_32_sample_edge(width):
    """255 rays: the wall at sample 0, then at 32 k - 1 and 32 k for k = 1 .. 127 -- every carry slot is written and read with an
    opaque sample as the last lane of the tile before it and as the first lane of its own"""
    S, n = Q.S_MAX, Q.edge_sweep_rays(Q.S_MAX)
    r = Q.reference("wall", n, S, "relu", "ndc", 25.0, ("w", "s", "d"))
    tag = f"wall sweep S={S} N={n}"
    w, d, lst, cnt, _ = run_fwd(width, r["x"], "ndc", 25.0, 1e-4)
    _check(w, r["fwd"]["w"], r["fwd"]["wcond"], Q.c_ops(S, width), tag, f"w{width} sweep weight")
    _check_structure(w, lst, cnt, 1e-4, S, tag)
    out, gz, gr = run_bwd(width, r["x"], "relu", "ndc", 25.0, r["cot"])
    _check_bwd(width, r, "relu", "ndc", 25.0, out, gz, gr, tag, "sweep")


@pytest.mark.parametrize("width", [32, 64])
def test_walls_at_tile_edges_and_in_consecutive_tiles(width):
    """opaque samples on a tile edge, in the first tile, in the last tile and in four consecutive tiles (T down to 1e-40): finite, bounded"""
    S = Q.WALLS_S
    for act, rt, scale in (("relu", "ndc", 25.0), ("softplus", "world", 1.0)):
        x = Q.walls_case(act, rt, scale)
        r = Q.reference_of(x, S, act, rt, scale, ("w", "s", "d"))
        assert 0.0 < float(r["fwd"]["w"][3, 191:].max()) < 1e-38 and 0.0 < float(r["fwd"]["w"][4, 101:].max()) < 1e-38
        tag = f"walls S={S} {act} {rt}"
        w, d, lst, cnt, _ = run_fwd(width, x, rt, scale, 1e-4)
        _check(w, r["fwd"]["w"], r["fwd"]["wcond"], Q.c_ops(S, width), tag, f"w{width} walls weight")
        _check_structure(w, lst, cnt, 1e-4, S, tag)
        for cs in (("w",), ("w", "s", "d")):
            rc = Q.reference_of(x, S, act, rt, scale, cs)
            out, gz, gr = run_bwd(width, x, act, rt, scale, rc["cot"])
            _check_bwd(width, rc, act, rt, scale, out, gz, gr, f"{tag} cot={'+'.join(cs)}", "walls")


@pytest.mark.parametrize("width", [32, 64])
def test_a_ray_does_not_depend_on_the_batch(width):
    """ray r of the N = 35 run, bit for bit, from the same ray run alone (and as a pair) with the same pre-fill: each ray's
    contributions come from one group of lanes in a fixed order"""
    for regime, S, act, rt, scale in (("wall", 65, "relu", "ndc", 25.0), ("mixed", 129, "softplus", "contract", 1.0),
                                      ("invalid", 33, "relu", "ndc", 1.0)):
        r = Q.reference(regime, N, S, act, rt, scale, ("w", "s", "d"))
        full = run_bwd(width, r["x"], act, rt, scale, r["cot"])
        wf, df, _, _, _ = run_fwd(width, r["x"], rt, scale, 1e-4)
        for rows in ([0], [16], [17], [34], [15, 16, 17]):
            part = run_bwd(width, r["x"], act, rt, scale, r["cot"], rows=rows)
            for a, b, name in zip(part, full, ("out", "g_z", "g_rays")):
                eq = torch.equal(a[:, :S], b[rows][:, :S]) if name == "out" else torch.equal(a, b[rows])
                assert eq, f"{regime} S={S} rays {rows}: {name} differs from the N = {N} run"
            xs = {k: v[rows].contiguous() for k, v in r["x"].items()}
            w1, d1, _, _, _ = run_fwd(width, xs, rt, scale, 1e-4)
            assert torch.equal(w1, wf[rows]) and torch.equal(d1, df[rows])


FIELD_SHAPES = ((17, 33), (3, 129))


def field_case():
    """the dynamic field's own forward (tools build, RDRF_FLAT from the environment) at FIELD_SHAPES: rays, z, sigma, weight, dists
    (tests/_det_child.py case)"""
    import rodynrf
    St = pkg("step")
    RU = pkg("ray_utils")
    torch.manual_seed(0)
    cfg = St.scene_config("nvidia", "stage0")
    dev = torch.device("cuda", 0)
    _, dy = St.build_fields(cfg, dev)
    data = St.SyntheticScene(cfg, dev)
    res = dict(scale=np.float32(dy.distance_scale), thres=np.float32(dy.rayMarch_weight_thres))
    with torch.no_grad():
        g = torch.Generator(device=dev).manual_seed(7)
        for p in dy.parameters():   # off the initial values, so that the densities are not all alike
            p.add_(torch.randn(p.shape, device=dev, generator=g) * 0.05 * (p.abs().mean() + 1e-3))
        for n, S in FIELD_SHAPES:
            ids = data.perm[:n]
            rays = RU.generate_rays(ids, data.poses, data.focal, cfg["H"], cfg["W"], ndc=True, near=1.0).detach().clone()
            jit = torch.rand(S, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
            xyz, z, valid = rodynrf.sampleXYZ(dy, rays, S, ray_type="ndc", is_train=True, jitter=jit)
            o = dy(rays, data.ts_of(ids), None, xyz, z, valid, is_train=True, ray_type="ndc")
            torch.cuda.synchronize()
            for k, t in (("rays", rays), ("z", o[8]), ("sigma", o[7]), ("weight", o[4]), ("dists", o[9])):
                res[f"{k}_{n}_{S}"] = t.detach().float().cpu().numpy()
    return res


def test_forward_entry_gives_the_dynamic_fields_own_weights(tmp_path):
    """width 32: the weights and dists of rdrf_selftest_ray_scan, bit for bit, from the sigmas the dynamic field's forward wrote -- on
    flat tiles (k_dyn_density_flat + k_ray_scan) and wave per ray (k_dyn_density: weight_round<32> in place), which must agree too"""
    got = {}
    for flat in ("0", "1"):
        res = run_twin(tmp_path, [CHILD, "case", "test_gpu_scan_primitives", "field_case"], lib=tools_lib(), extra_env={"RDRF_FLAT": flat},
                       timeout=300)
        got[flat] = {k: v.numpy() for k, v in res.items()}
    for n, S in FIELD_SHAPES:
        a, b = got["0"], got["1"]
        for k in ("rays", "z", "sigma", "weight", "dists"):
            assert np.array_equal(a[f"{k}_{n}_{S}"].view(np.uint32), b[f"{k}_{n}_{S}"].view(np.uint32)), f"{k} N={n} S={S}: flat on / off differ"
        x = {k: torch.from_numpy(a[f"{k}_{n}_{S}"]).contiguous() for k in ("rays", "z", "sigma")}
        assert float(x["sigma"].max()) > 0.0
        w, d, lst, cnt, _ = run_fwd(32, x, "ndc", float(a["scale"]), float(a["thres"]))
        assert np.array_equal(w.numpy().view(np.uint32), a[f"weight_{n}_{S}"].view(np.uint32)), f"N={n} S={S}: weights differ from the field's"
        assert np.array_equal(d.numpy().view(np.uint32), a[f"dists_{n}_{S}"].view(np.uint32)), f"N={n} S={S}: dists differ from the field's"
        _check_structure(w, lst, cnt, float(a["thres"]), S, f"field N={n} S={S}")


def test_entry_points_check_their_arguments():
    L = pkg()
    x = Q.generate("thin", 2, 8)
    z = x["z"].cuda()
    buf = torch.zeros(4096, device="cuda")
    ibuf = torch.zeros(4096, dtype=torch.int32, device="cuda")
    p, s = L.ptr(buf), L.stream_of(z)
    fwd, bwd = L.lib.rdrf_selftest_ray_scan, L.lib.rdrf_selftest_ray_scan_bwd
    assert fwd(32, None, None, None, 0, 8, 0, 25.0, 1e-4, None, None, None, None, None, s) == 0, "N = 0 is a no-op"
    assert bwd(64, None, None, None, None, 0, 8, 0, -10.0, 25.0, 0, None, None, None, None, None, None, s) == 0
    assert fwd(48, p, p, p, 2, 8, 0, 25.0, 1e-4, p, p, L.ptr(ibuf), L.ptr(ibuf), None, s) == -1
    assert fwd(32, p, p, p, 2, 0, 0, 25.0, 1e-4, p, p, L.ptr(ibuf), L.ptr(ibuf), None, s) == -1
    assert fwd(64, p, p, p, 2, 4097, 0, 25.0, 1e-4, p, p, L.ptr(ibuf), L.ptr(ibuf), None, s) == -1
    assert fwd(64, p, p, None, 2, 8, 0, 25.0, 1e-4, p, p, L.ptr(ibuf), L.ptr(ibuf), None, s) == -1
    assert fwd(32, p, p, p, 2, 8, 0, 25.0, 1e-4, p, p, L.ptr(ibuf), None, None, s) == -1
    assert bwd(16, p, p, p, p, 2, 8, 0, -10.0, 25.0, 0, None, None, None, p, None, None, s) == -1
    assert bwd(32, p, p, p, p, 2, 4097, 0, -10.0, 25.0, 0, None, None, None, p, None, None, s) == -1
    assert bwd(64, p, p, p, p, 2, 8, 0, -10.0, 25.0, 0, None, None, None, None, None, None, s) == -1
    assert bwd(64, p, p, None, p, 2, 8, 0, -10.0, 25.0, 0, None, None, None, p, None, None, s) == -1
    assert bwd(32, p, p, p, p, 2, 8, 2, -10.0, 25.0, 0, None, None, None, p, None, None, s) == -1
    assert b"selftest_ray_scan_bwd" in L.lib.rdrf_last_error()
    torch.cuda.synchronize()

