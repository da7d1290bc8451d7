"""Evaluation-path timings: python tools/eval_bench.py [--reps N]
  1. render_frame(maps=True) against render_frame on the stage-0 Balloon1-shaped frame (240 x 135, S = 115), interleaved
     A/B, host clock around each frame with a device synchronise;
  2. ssim on a 1080p pair (device events over repeated calls), and the float64 reference on the host (scipy's rgb_ssim
     restatement when scipy is installed, the numpy restatement of tests/test_gpu_render_maps.py otherwise).
  3. --motion [--stage stage0|final]: the motion legs instead (one JSON line): render_frame with all five motion maps against
     the composition of the public calls that produces the same maps (forward x 2, raw2outputs,
     get_forward_backward_scene_flow, induce_flow x 4, a torch sum), interleaved pairs; the cost of the five maps / of the
     three that need no scene-flow MLP over render_frame(maps=True) alone; the share of 32-sample tiles whose weights_d are
     all exactly 0 (they skip the MLP); flow_to_image at 240 x 135 and 1080p.
Prints one JSON line."""
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
S_ = importlib.import_module("robust-dynrf_amd.step")
R = importlib.import_module("robust-dynrf_amd.renderer")

reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 30
dev = torch.device("cuda", 0)
stage = sys.argv[sys.argv.index("--stage") + 1] if "--stage" in sys.argv else "stage0"
cfg = S_.scene_config("nvidia", stage)
tr = S_.Trainer(cfg, dev)
H, W, S, frame = cfg["H"], cfg["W"], cfg["n_samples"], 3
poses, focal = tr.pose_table().detach(), tr.focal()
focal = focal.detach() if torch.is_tensor(focal) else focal


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def motion_legs():
    from test_gpu_motion_maps import MOTION, _composition
    rt, T = cfg["ray_type"], poses.shape[0]
    f = float(focal) if torch.is_tensor(focal) else focal
    mtx = importlib.import_module("robust-dynrf_amd.ray_utils").pose_to_mtx(poses.float())
    cams = dict(H=H, W=W, focal=f, c2w_f=mtx[min(frame + 1, T - 1)].contiguous(), c2w_b=mtx[max(frame - 1, 0)].contiguous())
    gen = importlib.import_module("robust-dynrf_amd.ray_utils").generate_rays
    ids = torch.arange(H * W, device=dev) + frame * H * W
    rays = gen(ids, poses, f, H, W, ndc=rt == "ndc", near=1.0).detach()
    ts = torch.full((H * W,), 2.0 * frame / max(T - 1, 1) - 1.0, device=dev)
    frame_kw = dict(N_samples=S, ray_type=rt)
    native = lambda: R.render_frame(tr.st, tr.dy, poses, f, frame, H, W, maps=True, motion=True, **frame_kw)
    static3 = lambda: R.render_frame(tr.st, tr.dy, poses, f, frame, H, W, maps=True,
                                     motion=("flow_s_f", "flow_s_b", "delta_xyz"), **frame_kw)
    maps_only = lambda: R.render_frame(tr.st, tr.dy, poses, f, frame, H, W, maps=True, **frame_kw)

    def composed():   # the ten colour maps come out of its raw2outputs as well
        return _composition(tr.st, tr.dy, rays, ts, S, rt, cams)

    legs = {"native_5_motion_maps": native, "composition_of_public_calls": composed, "native_3_static_maps": static3,
            "render_frame_maps_only": maps_only}
    for fn in legs.values():
        for _ in range(3):
            fn()
    ms = {k: [] for k in legs}
    names = list(legs)
    for i in range(reps):   # rotate the order inside each round
        for k in names[i % len(names):] + names[:i % len(names)]:
            ms[k].append(timed(legs[k]))
    out = {"stage": stage, "frame": f"{W}x{H}", "S": S, "reps": reps}
    for k in names:
        out[k + "_ms_median"], out[k + "_ms_min"] = statistics.median(ms[k]), min(ms[k])
    out["native_slower_than_composition_in_pairs"] = sum(a > b for a, b in zip(ms[names[0]], ms[names[1]]))
    out["composition_over_native_median"] = out["composition_of_public_calls_ms_median"] / out["native_5_motion_maps_ms_median"]
    out["five_maps_added_over_maps_only"] = out["native_5_motion_maps_ms_median"] / out["render_frame_maps_only_ms_median"] - 1.0
    out["three_static_maps_added_over_maps_only"] = out["native_3_static_maps_ms_median"] / out["render_frame_maps_only_ms_median"] - 1.0
    w_d = composed()["w_d"]
    pad = (-S) % 32
    tiles = torch.nn.functional.pad(w_d, (0, pad)).view(H * W, -1, 32)
    out["tiles_with_all_zero_weights_d"] = float((tiles == 0).all(-1).float().mean())
    g = torch.Generator().manual_seed(1)
    for tag, (h, w) in (("240x135", (135, 240)), ("1080p", (1080, 1920))):
        fl = (torch.randn(h, w, 2, generator=g) * 3.0).to(dev)
        for _ in range(5):
            R.flow_to_image(fl)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(100):
            R.flow_to_image(fl)
        e1.record()
        torch.cuda.synchronize()
        out[f"flow_to_image_{tag}_ms"] = e0.elapsed_time(e1) / 100
    print(json.dumps(out))


if "--motion" in sys.argv:
    motion_legs()
    sys.exit(0)


def one(maps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    R.render_frame(tr.st, tr.dy, poses, focal, frame, H, W, N_samples=S, ray_type=cfg["ray_type"], maps=maps)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


for _ in range(3):
    one(False), one(True)
plain, maps = [], []
for i in range(reps):   # alternate the order inside each pair
    if i % 2:
        maps.append(one(True)), plain.append(one(False))
    else:
        plain.append(one(False)), maps.append(one(True))
res = {"frame": f"{W}x{H}", "S": S, "reps": reps,
       "render_frame_ms_median": statistics.median(plain), "render_frame_maps_ms_median": statistics.median(maps),
       "render_frame_ms_min": min(plain), "render_frame_maps_ms_min": min(maps)}
res["maps_over_plain_median"] = res["render_frame_maps_ms_median"] / res["render_frame_ms_median"]

g = torch.Generator().manual_seed(0)
a = torch.rand(1080, 1920, 3, generator=g)
b = (a + 0.05 * torch.randn(1080, 1920, 3, generator=g)).clamp(0, 1)
da, db = a.to(dev), b.to(dev)
for _ in range(5):
    R.ssim(da, db)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
n = 100
e0.record()
for _ in range(n):
    R.ssim(da, db)
e1.record()
torch.cuda.synchronize()
res["ssim_1080p_ms"] = e0.elapsed_time(e1) / n
m = None
e0.record()
for _ in range(n):
    m = R.ssim(da, db, return_map=True)
e1.record()
torch.cuda.synchronize()
res["ssim_1080p_with_map_ms"] = e0.elapsed_time(e1) / n
dev_mean = float(R.ssim(da, db))
try:
    import scipy.signal

    def host_ssim(x, y):
        filt = np.exp(-0.5 * ((np.arange(11) - 5) / 1.5) ** 2)
        filt /= filt.sum()
        conv = lambda z, f: scipy.signal.convolve2d(z, f, mode="valid")
        fn = lambda z: np.stack([conv(conv(z[..., i], filt[:, None]), filt[None, :]) for i in range(z.shape[-1])], -1)
        mu0, mu1 = fn(x), fn(y)
        s00 = np.maximum(0.0, fn(x * x) - mu0 * mu0)
        s11 = np.maximum(0.0, fn(y * y) - mu1 * mu1)
        s01 = fn(x * y) - mu0 * mu1
        s01 = np.sign(s01) * np.minimum(np.sqrt(s00 * s11), np.abs(s01))
        c1, c2 = 0.01 ** 2, 0.03 ** 2
        return float(np.mean((2 * mu0 * mu1 + c1) * (2 * s01 + c2) / ((mu0 * mu0 + mu1 * mu1 + c1) * (s00 + s11 + c2))))
    res["host_reference"] = "scipy.signal.convolve2d"
except ImportError:
    from test_gpu_render_maps import _ssim_f64
    host_ssim = lambda x, y: _ssim_f64(x, y)[1]
    res["host_reference"] = "numpy restatement"
x64, y64 = a.numpy().astype(np.float64), b.numpy().astype(np.float64)
t0 = time.perf_counter()
host = host_ssim(x64, y64)
res["ssim_1080p_host_ms"] = (time.perf_counter() - t0) * 1e3
res["ssim_1080p_rel_diff_device_vs_host"] = abs(dev_mean - host) / abs(host)
print(json.dumps(res))
