"""render Mpix/s (whole frame and 512-ray chunks) + the per-kernel forward times of a no-grad pass: python tools/render_bench.py
[whole | chunk512 | masked] [--stage=final].  `masked`: whole frames through the masked render (render_rays(alpha_masks=...))
with synthetic depth-slab masks of 100 %, 25 % and 5 % occupancy on both fields, interleaved with the unmasked render."""
import ctypes as C
import importlib
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
S_ = importlib.import_module("robust-dynrf_amd.step")
R = importlib.import_module("robust-dynrf_amd.renderer")
L = importlib.import_module("robust-dynrf_amd._lib")
stage = "final" if "--stage=final" in sys.argv else "stage0"
cfg = S_.scene_config("nvidia", stage)
dev = torch.device("cuda", 0)
tr = S_.Trainer(cfg, dev)
H, W = cfg["H"], cfg["W"]
ids = torch.arange(H * W, device=dev)
with torch.no_grad():
    rays_f = tr.rays_for(ids + 3 * H * W).detach()
ts_f = tr.data.ts_of(ids + 3 * H * W)


def frame(chunk):
    for c0 in range(0, H * W, chunk):
        R.render_rays(tr.st, tr.dy, rays_f[c0:c0 + chunk], ts_f[c0:c0 + chunk], N_samples=cfg["n_samples"], ray_type=cfg["ray_type"])


def masked_leg(rounds=12):
    """frame times (HIP events around one whole-frame call) of the unmasked render and of the masked render at three
    occupancies, one frame of each per round so that drift hits all alike; then one profiled frame of each"""
    A = importlib.import_module("robust-dynrf_amd.alpha")
    S, rt = cfg["n_samples"], cfg["ray_type"]
    G2 = 200
    masks = {}
    for pct in (100, 25, 5):   # the first pct % of the depth axis occupied, over the field's own box
        vol = torch.zeros(G2, 4, 4, 2)
        vol[:max(1, round(G2 * pct / 100))] = 1
        masks[pct] = tuple(A.AlphaGridMask(dev, f.aabb, vol, 2) for f in (tr.st, tr.dy))
    kept = torch.zeros(2, dtype=torch.int64, device=dev)
    legs = [("unmasked", None)] + [(f"masked {pct:3d} %", masks[pct]) for pct in (100, 25, 5)]

    def run(m):
        return R.render_rays(tr.st, tr.dy, rays_f, ts_f, N_samples=S, ray_type=rt, alpha_masks=m, kept=kept if m else None)

    times = {name: [] for name, _ in legs}
    counts = {}
    for name, m in legs:   # warm-up: workspaces, packed images
        run(m)
        counts[name] = kept.cpu().tolist() if m else None
    torch.cuda.synchronize()
    for _ in range(rounds):
        for name, m in legs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(m)
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1))
    print(f"{stage}: grid {cfg['grid']}, {H} x {W} frame, S = {S}, {H * W * S} samples; {rounds} interleaved rounds, ms per frame")
    for name, _ in legs:
        t = sorted(times[name])
        k = "" if counts[name] is None else f"  kept (static, dynamic) = {counts[name]}"
        print(f"  {name:13s} median {t[len(t) // 2]:7.3f}  min {t[0]:7.3f}  max {t[-1]:7.3f}{k}")
    L.lib.rdrf_prof_enable(1)
    for name, m in legs:
        L.lib.rdrf_prof_reset()
        run(m)
        torch.cuda.synchronize()
        print(f"  kernels, {name}:")
        for k in ("sample_ndc", "time_branch", "mask_keep", "static_density", "static_density_list", "static_scan", "dyn_density",
                  "dyn_density_list", "ray_scan", "static_app", "dyn_app", "composite"):
            ms, c = C.c_double(), C.c_int()
            L.lib.rdrf_prof_get(k.encode(), C.byref(ms), C.byref(c))
            if c.value:
                print(f"    {k:20s} {ms.value:7.3f} ms")
    L.lib.rdrf_prof_enable(0)


which = [a for a in sys.argv[1:] if not a.startswith("--")]
if which and which[0] == "masked":
    masked_leg()
    sys.exit(0)
chunks = {"whole": (H * W,), "chunk512": (512,)}.get(which[0] if which else "", (H * W, 4096, 512))
for chunk in chunks:
    frame(chunk)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 5 if chunk > 512 else 2
    for _ in range(n):
        frame(chunk)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / n
    print(f"chunk {chunk:6d}: {H * W / dt / 1e6:6.3f} Mpix/s  {dt * 1e3:7.3f} ms/frame")
if 512 in chunks:   # the native chunk loop (rdrf_render_chunks_fwd), one stream and four
    for ns in (1, 4, 8, 16):
        R.render_chunks(tr.st, tr.dy, rays_f, ts_f, 512, N_samples=cfg["n_samples"], ray_type=cfg["ray_type"], streams=ns)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            R.render_chunks(tr.st, tr.dy, rays_f, ts_f, 512, N_samples=cfg["n_samples"], ray_type=cfg["ray_type"], streams=ns)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / 3
        print(f"native chunk loop, 512-ray chunks, {ns} stream(s): {H * W / dt / 1e6:6.3f} Mpix/s  {dt * 1e3:7.3f} ms/frame")
L.lib.rdrf_prof_enable(1)
L.lib.rdrf_prof_reset()
for chunk in chunks:
    frame(chunk)
torch.cuda.synchronize()
for k in ("sample_ndc", "static_density", "static_app", "time_branch", "dyn_density", "ray_scan", "dyn_app", "composite", "render_fused"):
    ms, c = C.c_double(), C.c_int()
    L.lib.rdrf_prof_get(k.encode(), C.byref(ms), C.byref(c))
    if c.value:
        print(f"  {k:16s} {ms.value:7.3f} ms ({c.value} launches, {ms.value / c.value * 1e3:7.1f} us each)")
L.lib.rdrf_prof_enable(0)
