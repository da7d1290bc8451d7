"""CPU-side checks of the surface hits (render_hits / rdrf_render_hits_fwd, rdrf_hits_from_planes): the float64 reference of
tests/_hits_prim.py against the visibility reference it inverts, its ends, the inputs of the GPU tests, an fp32 evaluation of
the kernel's formulas against the GPU file's own bounds, the ABI additions, the package surface, the argument checks (which
come before any device work) and the vertex-only PLY."""
import ctypes as C
import hashlib
import inspect
import os
import re

import numpy as np
import pytest
import torch

import _hits_prim as H
import _track_vis_prim as P

from _util import pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T8 = H.TAUS[8]


@pytest.mark.parametrize("rt", ["ndc", "contract"])
@pytest.mark.parametrize("S", [2, 13, 65, 129])
def test_reference_inverts_the_visibility(rt, S):
    rays, z, ss, sd, b = H.planes(rt, 257, S)
    dists = H.dists_of(z, rays, H.DISTANCE_SCALE[rt])
    prev_z, prev_hit = None, None
    for tau in T8:
        r = H.hits(z, dists, ss, sd, b, tau)
        hit = r["hit"]
        # z_hit fed back into the visibility returns L.  visibility() multiplies the plain product T_j where the hits take the
        # running minimum m_j; the two differ by the 1e-10 a sample without density adds (T rises by it, m does not), so the
        # visibility is scaled by the reference's own m_j / T_j, which is 1 - O(S 1e-10)
        vis, jv = P.visibility(z, dists, ss, sd, b, torch.where(hit, r["z"], z[:, 0].double()))
        Tj = r["T"].gather(1, r["j"].clamp(min=0)[:, None])[:, 0]
        assert bool((jv == r["j"])[hit & (r["d"] > 0)].all())
        assert float(r["m_j"].sub(Tj).abs().div(Tj).max()) <= S * 1.01e-10
        assert float((vis * (r["m_j"] / Tj) - r["L"]).abs()[hit].max() if bool(hit.any()) else 0.0) <= 1e-12
        # the bracket
        j = r["j"][hit]
        zj, zn = z.double()[hit].gather(1, j[:, None])[:, 0], z.double()[hit].gather(1, (j + 1)[:, None])[:, 0]
        assert bool(((zj <= r["z"][hit]) & (r["z"][hit] <= zn)).all()) and bool((j < S - 1).all())
        # a miss: the last sample, owner 0
        assert bool((r["z"][~hit] == z[~hit, -1].double()).all()) and bool((r["owner"][~hit] == 0).all())
        assert bool(((r["owner"] >= 0) & (r["owner"] <= 1)).all())
        # monotone in tau
        if prev_z is not None:
            assert bool((r["z"] >= prev_z).all()) and bool((hit.int() <= prev_hit.int()).all())
        prev_z, prev_hit = r["z"], hit


def _one_ray(S=13):
    rays = torch.tensor([[0.1, -0.2, -1.0, 0.05, 0.02, 2.0]])
    z = torch.linspace(0.0, 1.0, S)[None].float()
    return rays, z, H.dists_of(z, rays, 25.0)


def test_reference_ends():
    S = 13
    rays, z, dists = _one_ray(S)
    ds = float(dists[0, 0])
    zero, one = torch.zeros(1, S), torch.ones(1, S)
    # an empty ray misses every level
    for tau in T8:
        r = H.hits(z, dists, zero, zero, zero, tau)
        assert not bool(r["hit"][0]) and float(r["z"][0]) == float(z[0, -1]) and int(r["j"][0]) == -1
    # an opaque first sample: j = 0, the hit in its first thousandth
    first = zero.clone()
    first[0, 0] = 1e5 / ds
    r = H.hits(z, dists, first, zero, zero, 0.9)
    assert bool(r["hit"][0]) and int(r["j"][0]) == 0 and 0.0 < float(r["z"][0]) < 1e-3 * float(z[0, 1]) and float(r["owner"][0]) == 0.0
    # a crossing on a sample: a factor a hair under 1/2 (1e-9 relative, past the + 1e-10) meets L = 1/2 at the interval's very end
    half = zero.clone().double()
    half[0, 3] = np.log(2.0) / float(dists[0, 3]) * (1.0 + 1e-9)
    F = P.factor(zero.double(), half, one.double(), dists)
    assert 0.0 < 0.5 - float(F[0, 3]) <= 1e-9
    r = H.hits(z, dists, zero, half, one, 0.5)
    assert bool(r["hit"][0]) and int(r["j"][0]) == 3
    assert abs(float(r["z"][0]) - float(z[0, 4])) <= 1e-8 * float(z[0, 4] - z[0, 3])
    # a level only the last, zero-width sample could cross: its density meets dists = 0
    last = zero.clone()
    last[0, S - 1] = 1e5
    for tau in T8:
        assert not bool(H.hits(z, dists, last, zero, zero, tau)["hit"][0])
    # b in {0, 1}: the other field does not count; one sigma zero: the closed form of a single exponential
    sig = zero.clone()
    sig[0, 5] = 3.0 / float(dists[0, 5])
    for b, ss, sd, own in ((one, zero, sig, 1.0), (zero, sig, zero, 0.0)):
        r = H.hits(z, dists, ss, sd, b, 0.5)
        want = float(z[0, 5]) + np.log(2.0 / (1.0 + 2e-10)) / 3.0 * float(z[0, 6] - z[0, 5])
        assert bool(r["hit"][0]) and int(r["j"][0]) == 5 and abs(float(r["z"][0]) - want) <= 1e-7 and float(r["owner"][0]) == own
        other = H.hits(z, dists, sd, ss, b, 0.5)          # the density in the field the blending switches off: a miss
        assert not bool(other["hit"][0])
    # NaN: behind the crossing no effect, at or before it NaN and no hit
    sn = sig.clone()
    sn[0, 8] = float("nan")
    r = H.hits(z, dists, zero, sn, one, 0.5)
    assert bool(r["hit"][0]) and int(r["j"][0]) == 5
    r = H.hits(z, dists, zero, sn, one, 0.99)
    assert not bool(r["hit"][0]) and bool(r["nan"][0]) and bool(torch.isnan(r["z"][0]))


def test_inputs_exercise_the_solver_and_stay_above_the_slope_floor():
    """the seeded planes of test_gpu_hits.py: a stated share of the hitting rays crosses BETWEEN samples with both alphas
    non-zero (no closed form), and at most FLOOR_CAP of them lie under the slope floor of the depth check"""
    for rt in ("ndc", "contract"):
        both = hits = under = 0
        for S in (63, 64, 65, 129):
            rays, z, ss, sd, b = H.planes(rt, 257, S)
            dists = H.dists_of(z, rays, H.DISTANCE_SCALE[rt])
            for tau in T8:
                r = H.hits(z, dists, ss, sd, b, tau)
                hit = r["hit"]
                j = r["j"].clamp(min=0)[:, None]
                g = lambda t: t.double().gather(1, j)[:, 0]
                inner = hit & (r["d"] > 0) & (r["d"] < g(dists))
                two = inner & (g(ss) > 0) & (g(sd) > 0) & (g(b) > 0) & (g(b) < 1)
                width = g(torch.cat([z[:, 1:], z[:, -1:]], -1)) - g(z)
                hits += int(hit.sum())
                both += int(two.sum())
                under += int((hit & (r["slope"] * width < H.SLOPE_FLOOR * r["m_j"])).sum())
        assert hits >= 2000 and both >= 0.3 * hits, (rt, hits, both)
        assert under <= H.FLOOR_CAP * hits, (rt, hits, under)


@pytest.mark.parametrize("rt", ["ndc", "contract"])
@pytest.mark.parametrize("S", [2, 64, 65, 129])
def test_an_fp32_evaluation_lies_inside_the_gpu_bounds(rt, S):
    """the kernel's formulas in fp32 torch (a sequential product in the place of the scan) through the very checks
    test_gpu_hits.py applies to the kernel: residual, depth, bracket, flags, owner"""
    pl = H.planes(rt, 257, S)
    got = H.emulate_fp32(*pl, T8, H.DISTANCE_SCALE[rt])
    worst, n_hit, n_floor, n_clear, n_all = H.check_against_reference(rt, pl, got, T8, f"fp32 torch {rt} S={S}")
    assert worst <= 1.0 and n_clear >= 0.9 * n_all
    assert bool((got["z"][1:] >= got["z"][:-1]).all()) and bool((got["hit"][1:].int() <= got["hit"][:-1].int()).all())


def test_abi_additions():
    L = pkg()
    hdr = open(os.path.join(ROOT, "include", "rodynrf.h")).read()
    for sym in ("rdrf_hits_from_planes", "rdrf_render_hits_ws_bytes", "rdrf_render_hits_fwd"):
        assert re.search(r"\b" + sym + r"\s*\(", hdr), sym
        assert sym in L.SIGNATURES and hasattr(L.lib, sym), sym
    assert "#define RDRF_ABI_VERSION 6" in hdr and L.lib.rdrf_abi_version() == 6 == L.ABI_VERSION
    body = re.search(r"typedef struct RdrfHits \{(.*?)\} RdrfHits;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [d.split()[-1].strip("* ") for d in body.split(";") if d.strip()]
    assert names == [f for f, _ in L.HitsC._fields_] == list(L.HIT_OUTPUTS) and C.sizeof(L.HitsC) == 32
    assert C.sizeof(L.TrackCamsC) == 32 and C.sizeof(L.TracksC) == 24 and C.sizeof(L.RenderMapsC) == 80   # untouched
    f, g = L.lib.rdrf_render_hits_ws_bytes, L.lib.rdrf_render_workspace_bytes
    for N in (1, 33, 4096):
        for S in (1, 13, 65, 440):
            assert int(f(N, S)) >= int(g(N, S)) > 0
    assert int(f(4096, 65)) > int(f(33, 65)) > int(f(1, 65)) and int(f(33, 440)) > int(f(33, 13))


def test_package_surface():
    import rodynrf
    for name in ("render_hits", "hit_view", "hits_from_planes", "render_hit_tracks", "point_cloud", "contract_to_world"):
        assert name in rodynrf.__all__ and hasattr(rodynrf, name), name
    sig = inspect.signature(rodynrf.render_hits)
    assert list(sig.parameters) == ["tensorf_static", "tensorf", "rays", "ts", "tau", "N_samples", "ray_type", "maps"]
    assert sig.parameters["tau"].default == 0.5 and sig.parameters["maps"].default is False
    sig = inspect.signature(rodynrf.hit_view)
    assert list(sig.parameters)[:9] == ["tensorf_static", "tensorf", "c2w", "focal", "H", "W", "t", "tau", "N_samples"]
    sig = inspect.signature(rodynrf.point_cloud)
    assert list(sig.parameters)[:11] == ["tensorf_static", "tensorf", "c2w", "focal", "H", "W", "t", "tau", "space", "min_owner",
                                         "max_owner"]
    assert sig.parameters["space"].default == "field"
    assert list(inspect.signature(rodynrf.render_hit_tracks).parameters)[-1] == "tau"
    assert inspect.signature(rodynrf.write_ply).parameters["faces"].default is None
    assert os.path.exists(os.path.join(ROOT, "tools", "export_points.py"))
    # contract_to_world inverts the samplers' contraction
    p = torch.tensor([[0.3, -0.2, 0.9], [3.0, -1.0, 0.5], [-7.0, 2.0, 40.0]], dtype=torch.float64)
    n = p.abs().amax(-1, keepdim=True)
    c = torch.where(n > 1, (2.0 - 1.0 / n) * (p / n), p)
    assert float((rodynrf.contract_to_world(c) - p).abs().max()) <= 1e-9


def test_argument_errors_come_before_device_work():
    """every tensor is on the CPU: a call that got as far as the device would raise RdrfError (no CPU fallback)"""
    import rodynrf
    rays, ts = torch.zeros(4, 6), torch.zeros(4)
    for bad in (0.0, 1.0, -0.1, float("nan"), (0.5, 0.4), (0.5, 0.5), (), tuple(0.1 * k for k in range(1, 10))):
        with pytest.raises(ValueError):
            rodynrf.render_hits(None, None, rays, ts, tau=bad)
        with pytest.raises(ValueError):
            rodynrf.hits_from_planes(rays, ts[:, None], ts[:, None], ts[:, None], ts[:, None], tau=bad)
    with pytest.raises(NotImplementedError):
        rodynrf.render_hits(None, None, rays, ts, ray_type="world")
    with pytest.raises(NotImplementedError):
        rodynrf.hit_view(None, None, torch.eye(3, 4), 10.0, 4, 4, 0.0, ray_type="world")
    with pytest.raises(ValueError):
        rodynrf.render_hits(None, None, rays, ts, maps=("nope",))
    with pytest.raises(ValueError):
        rodynrf.render_hit_tracks(None, None, torch.zeros(3, 9), 10.0, 0, torch.zeros(2, 2), 4, 4, tau=(0.2, 0.4))
    # the C entry points refuse the same before touching the device
    L = pkg()
    PS, PD, cs, cd = L.RdrfStaticParams(), L.RdrfDynamicParams(), L.RdrfFieldCfg(), L.RdrfFieldCfg()
    out = L.HitsC()

    def taus_of(v):
        return (C.c_float * max(len(v), 1))(*v)

    def render(N=0, S=13, taus=(0.5,), n_tau=None, rt=(0, 0), out_=out):
        cs.ray_type, cd.ray_type = rt
        return L.lib.rdrf_render_hits_fwd(C.byref(PS), C.byref(cs), C.byref(PD), C.byref(cd), None, None, N, S, 0.0, 1.0,
                                          taus_of(taus), len(taus) if n_tau is None else n_tau, None,
                                          None if out_ is None else C.byref(out_), None, 0, None)

    def planes(N=0, S=13, taus=(0.5,), n_tau=None, rt=0):
        return L.lib.rdrf_hits_from_planes(None, None, None, None, None, N, S, rt, 1.0, taus_of(taus),
                                           len(taus) if n_tau is None else n_tau, C.byref(out), None)

    assert render() == 0 and render(rt=(1, 1)) == 0 and planes() == 0 and planes(rt=1) == 0       # N == 0: a no-op
    nine = tuple(0.1 * k for k in range(1, 10))
    for kw in (dict(rt=(2, 2)), dict(rt=(0, 1)), dict(S=0), dict(N=-1), dict(taus=(0.0,)), dict(taus=(1.0,)), dict(taus=(0.5, 0.5)),
               dict(taus=(0.6, 0.5)), dict(taus=nine), dict(n_tau=0), dict(out_=None), dict(N=3)):
        assert render(**kw) == -1, kw
        assert b"render_hits" in L.lib.rdrf_last_error(), kw
    for kw in (dict(rt=2), dict(S=0), dict(N=-1), dict(taus=(0.0,)), dict(taus=(0.6, 0.5)), dict(taus=nine), dict(n_tau=0), dict(N=3)):
        assert planes(**kw) == -1, kw
        assert b"hits_from_planes" in L.lib.rdrf_last_error(), kw


def test_vertex_only_ply_round_trip_and_faced_bytes(tmp_path):
    import rodynrf
    g = torch.Generator().manual_seed(5)
    v = torch.randn(17, 3, generator=g)
    c = torch.randint(0, 256, (17, 3), generator=g, dtype=torch.uint8)
    path = str(tmp_path / "cloud.ply")
    rodynrf.write_ply(path, v, None, colors=c)
    back = rodynrf.read_ply(path)
    assert back["faces"].shape == (0, 3) and back["faces"].dtype == np.int32 and back["normals"] is None
    assert np.array_equal(back["verts"], v.numpy()) and np.array_equal(back["colors"], c.numpy())
    assert b"element face" not in open(path, "rb").read()
    rodynrf.write_ply(path, v[:0])
    assert rodynrf.read_ply(path)["verts"].shape == (0, 3)
    # a faced mesh: the bytes of the writer as it was before faces became optional (recorded from that writer)
    verts = (torch.arange(12, dtype=torch.float32).reshape(4, 3) * 0.25 - 1.0)
    faces = torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int32)
    normals = torch.flip(verts, dims=(1,))
    colors = (torch.arange(12).reshape(4, 3) * 20).to(torch.uint8)
    rodynrf.write_ply(path, verts, faces, normals=normals, colors=colors)
    assert hashlib.sha256(open(path, "rb").read()).hexdigest() == FACED_SHA256
    rodynrf.write_ply(path, verts, faces)
    assert hashlib.sha256(open(path, "rb").read()).hexdigest() == FACED_PLAIN_SHA256


FACED_SHA256 = "03d12f0737ae0597bc947da398a3666cd66039fde1b2be8c9cb2b0ffc5961d7c"
FACED_PLAIN_SHA256 = "fb6e1ca99ff07d87860c274d4b574c989e617499e246985e068dab7b74d9c8ff"
