"""CPU checks of the point tracks: the header, the binding and the built library agree on the new symbols, the workspace
size, the argument validation of the C entry point and of track_points (both refuse before any device work), the mirrored
reference method, the kernels' register budget and the fixture tests/golden/tracks.npz."""
import ctypes as C
import importlib
import importlib.util
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from _util import pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("rdrf_track_points_fwd", "rdrf_track_ws_bytes", "rdrf_render_track_seeds_fwd")


def test_header_binding_and_library_agree():
    L = pkg()
    hdr = open(os.path.join(ROOT, "include", "rodynrf.h")).read()
    for sym in SYMS:
        assert re.search(r"\b" + sym + r"\(", hdr), sym
        assert sym in L.SYMBOLS, sym
        assert hasattr(L.lib, sym), sym
    assert "#define RDRF_ABI_VERSION 6" in hdr and L.lib.rdrf_abi_version() == 6
    # the two new structs against the header's field lists
    for name, cls in (("RdrfTrackCams", L.TrackCamsC), ("RdrfTracks", L.TracksC)):
        body = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + ";", hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = []
        for decl in body.split(";"):
            if decl.strip():
                names += [n.split()[-1].strip("* ") for n in (decl.split(",") if "*" not in decl else [decl])]
        assert names == [f for f, _ in cls._fields_], (name, names)
    assert C.sizeof(L.TrackCamsC) == 32 and C.sizeof(L.TracksC) == 24


def test_package_surface():
    import rodynrf
    for name in ("Tracks", "track_points", "render_tracks"):
        assert name in rodynrf.__all__ and hasattr(rodynrf, name), name
    assert rodynrf.Tracks._fields == ("points", "pixels", "disp", "frames_offset")
    sig = inspect.signature(rodynrf.track_points)
    assert list(sig.parameters) == ["tensorf", "pts", "ts", "n_fwd", "n_bwd", "T", "cameras", "focal", "H", "W", "ray_type"]
    sig = inspect.signature(rodynrf.render_tracks)
    assert list(sig.parameters) == ["tensorf_static", "tensorf", "poses9", "focal", "frame", "pixels", "H", "W", "span",
                                    "N_samples", "ray_type"]


def test_point_single_has_the_reference_signature():
    import rodynrf
    fn = rodynrf.TensorVMSplit_TimeEmbedding.get_forward_backward_scene_flow_point_single
    assert list(inspect.signature(fn).parameters) == ["self", "pts_map_NDC", "t_sampled"]
    # the reference's get_forward_backward_scene_flow_point cannot run and is not mirrored
    assert not hasattr(rodynrf.TensorVMSplit_TimeEmbedding, "get_forward_backward_scene_flow_point")


def test_workspace_bytes_is_monotone():
    L = pkg()
    f = L.lib.rdrf_track_ws_bytes
    sizes = [[int(f(M, K)) for K in (1, 2, 9, 25, 100, 1000)] for M in (0, 1, 31, 32, 33, 70, 4096, 65569, 1 << 22)]
    assert all(v > 0 for row in sizes for v in row)
    for row in sizes:
        assert row == sorted(row)
    for col in zip(*sizes):
        assert list(col) == sorted(col)


def _call(L, ray_type=0, n_fwd=1, n_bwd=1, K=None, with_out=True, pix=False, M=0, p0=None):
    P = L.RdrfDynamicParams()
    cfg = L.RdrfFieldCfg()
    for i, v in enumerate((-1, -1, -1, 1, 1, 1)):
        cfg.aabb[i] = v
    cfg.ray_type = ray_type
    cams = None
    if K is not None:
        cams = L.TrackCamsC(4, 4, K, 1, 1)   # (pointers are not dereferenced: every check below fails before a launch)
    out = L.TracksC(None, 1 if pix else None, None)
    return L.lib.rdrf_track_points_fwd(C.byref(P), C.byref(cfg), p0, None, M, n_fwd, n_bwd, C.c_float(0.1),
                                       None if cams is None else C.byref(cams), C.byref(out) if with_out else None, None, 0, None)


def test_c_entry_validates_its_arguments():
    L = pkg()
    assert _call(L) == 0                                   # M == 0: a no-op once the arguments are sound
    assert _call(L, K=3) == 0
    for kw, word in ((dict(n_fwd=-1), "step counts"), (dict(n_bwd=-2), "step counts"), (dict(K=4), "cameras"),
                     (dict(K=2), "cameras"), (dict(ray_type=2), "ndc or contract"), (dict(with_out=False), "bad arguments"),
                     (dict(pix=True), "need the cameras"), (dict(M=-1), "bad arguments"), (dict(M=5), "no seed")):
        assert _call(L, **kw) == -1, kw
        assert word in L.lib.rdrf_last_error().decode(), (kw, L.lib.rdrf_last_error())


def test_track_points_validates_before_device_work():
    import rodynrf
    p, t = torch.zeros(4, 3), torch.zeros(4)
    cams = torch.zeros(3, 3, 4)
    with pytest.raises(NotImplementedError):
        rodynrf.track_points(None, p, t, 1, 1, 12, ray_type="world")
    with pytest.raises(NotImplementedError):
        rodynrf.render_tracks(None, None, torch.zeros(6, 9), 10.0, 0, torch.zeros(2, 2), 4, 4, ray_type="world")
    for kw in (dict(n_fwd=-1, n_bwd=0), dict(n_fwd=0, n_bwd=-1)):
        with pytest.raises(ValueError, match="step counts"):
            rodynrf.track_points(None, p, t, T=12, **kw)
    with pytest.raises(ValueError, match="cameras must be"):
        rodynrf.track_points(None, p, t, 2, 1, 12, cameras=cams, focal=10.0, H=4, W=4)
    with pytest.raises(ValueError, match="focal, H and W"):
        rodynrf.track_points(None, p, t, 1, 1, 12, cameras=cams)
    with pytest.raises(ValueError, match="T < 2"):
        rodynrf.track_points(None, p, t, 1, 0, 1)
    with pytest.raises(ValueError):
        rodynrf.track_points(None, p, torch.zeros(5), 1, 0, 12)
    with pytest.raises(rodynrf.RdrfError):   # no CPU fallback
        rodynrf.track_points(None, p, t, 1, 1, 12)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("c++filt") is None, reason="needs hipcc")
def test_track_kernels_do_not_spill():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    rows = {subprocess.run(["c++filt", r["name"]], capture_output=True, text=True).stdout.strip(): r
            for r in kr.table(os.path.join(kr.CSRC, "rdrf_track.hip"))}
    for w in ("k_track_points(", "k_track_seeds("):
        hit = [(n, r) for n, r in rows.items() if w in n]
        assert len(hit) == 1, (w, list(rows))
        name, r = hit[0]
        assert int(r["VGPRs"]) <= 256, (name, r["VGPRs"])
        assert int(r["VGPRs Spill"]) == 0, (name, r["VGPRs Spill"])
        assert int(r["ScratchSize [bytes/lane]"]) == 0, (name, r["ScratchSize [bytes/lane]"])
        assert int(r["Occupancy [waves/SIMD]"]) >= 2, (name, r["Occupancy [waves/SIMD]"])


def test_tracks_fixture_is_worth_having():
    from _util import GOLDEN
    path = os.path.join(GOLDEN, "tracks.npz")
    assert os.path.getsize(path) < 1 << 20
    z = np.load(path)
    M, nf, nb = int(z["meta.M"]), int(z["meta.n_fwd"]), int(z["meta.n_bwd"])
    K = nb + 1 + nf
    assert (M, nf, nb) == (70, 5, 3) and z["cams"].shape == (K, 3, 4) and z["t0"].shape == (M,)
    for rt in ("ndc", "contract"):
        pts = z[rt + ".chain.pts"]
        assert pts.shape == (M, K, 3) and np.isfinite(pts).all()
        assert np.array_equal(pts[:, nb], z[rt + ".p0"])
        assert np.median(np.abs(pts[:, 1:] - pts[:, :-1])) >= 0.005          # the chain moves
        for n in ("pts_f", "pts_b", "sf_f", "sf_b"):
            assert z[f"{rt}.single.{n}"].shape == (M, 3)
    assert z["ndc.chain.pix"].shape == (M, K, 2) and z["ndc.chain.disp"].shape == (M, K)
    hi = np.float32(2.0 - 1e-6)
    c = z["contract.chain.pts"]
    assert (np.abs(np.delete(c, nb, 1)) == hi).any()              # the step clamp fires
    assert (z["ndc.p0"][:, 2] >= 1 - 1e-6).sum() >= 3            # NDC2world's clamp
    # the times of every slot stay inside the video
    T = int(z["meta.T"])
    assert (z["t0"] - nb * 2 / (T - 1) >= -1 - 1e-6).all() and (z["t0"] + nf * 2 / (T - 1) <= 1 + 1e-6).all()


def _fit_scene():
    spec = importlib.util.spec_from_file_location("fit_scene", os.path.join(ROOT, "tools", "fit_scene.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_fit_scene_query_grid():
    fs = _fit_scene()
    for H, W in ((1, 1), (3, 5), (12, 16), (24, 32), (5, 40), (40, 5)):
        for n in sorted({1, 2, 3, 7, 12, 40, H * W - 1, H * W, H * W + 9} - {0}):
            q = fs.track_queries(n, H, W)
            want = min(n, H * W)
            assert q.shape == (want, 2) and q.dtype == torch.int64, (H, W, n)
            assert int(q[:, 0].min()) >= 0 and int(q[:, 0].max()) < W and int(q[:, 1].min()) >= 0 and int(q[:, 1].max()) < H
            assert len({(int(x), int(y)) for x, y in q}) == want, (H, W, n)     # distinct pixels
    q = fs.track_queries(12, 24, 32)        # a 3 x 4 lattice of cell centres, row-major
    assert q.tolist() == [[x, y] for y in (4, 12, 20) for x in (4, 12, 20, 28)]


def test_fit_scene_summary_line():
    import json
    fs = _fit_scene()
    ev = dict(psnr=[20.0, 22.0], ssim=[0.5, 0.7], psnr_mean=21.0, ssim_mean=0.6)
    metrics = dict(iterations=3, grid=[17, 19, 11], n_samples=13, loss=[(0, 1.0)], train=ev, heldout=ev,
                   alpha_mask=dict(grid=[8, 8, 8], static=dict(occupied=3, total=512, fraction=3 / 512)), train_masked=ev,
                   tracks=dict(n=12, frame=2))
    out = fs.summary(metrics)
    assert "loss" not in out and out["train"] == dict(psnr_mean=21.0, ssim_mean=0.6) == out["heldout"] == out["train_masked"]
    assert out["tracks"] == dict(n=12, frame=2) and out["alpha_mask"] == metrics["alpha_mask"] and out["iterations"] == 3
    json.dumps(out)
