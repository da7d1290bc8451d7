"""Time the surface hits (render_hits / rdrf_render_hits_fwd) at the render shape bench.py uses -- one H x W frame of the
Nvidia config at the final stage's grid and sample count -- against what a user writes without them:
    (a) render_rays(maps=True), then the planes the median depth needs (sampleXYZ and two forward(rgb=False): render_rays
        hands out no per-sample plane), the compositor's factor, cumprod and searchsorted in torch
    (b) render_hits(maps=True)            the render's maps and the hits from its own planes
    (c) render_hits(maps=False)           the density-only path
    (k) hits_from_planes                  k_render_hits alone, on forward()'s planes: its time and the bytes per second of the
                                          four [N][S] fp32 planes it reads
Interleaved rounds (a, b, c, k, a, ...), HIP events around each leg on the current stream after a warm-up, medians and the
min-max spread.

    python tools/bench_hits.py [--rounds 15] [--tau 0.5] [--out FILE]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--tau", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import rodynrf
    from _gpu_util import COMMON
    dev = "cuda"
    torch.manual_seed(11)
    cfg = rodynrf.scene_config("nvidia")
    _, grid, S = rodynrf.resolution_stages(cfg)[-1]
    H, W, rt = cfg["H"], cfg["W"], "ndc"
    # density_shift -2: a ray's optical depth is of order 5, as in tests/test_gpu_track_vis.py
    kw = dict(COMMON, near_far=[0.0, 1.0], density_shift=-2.0, fea2denseAct="softplus")
    aabb = torch.tensor(cfg["aabb"])
    st = rodynrf.TensorVMSplit(aabb, grid, 12, dev, shadingMode="MLP_Fea", fea_pe=2, **kw)
    dy = rodynrf.TensorVMSplit_TimeEmbedding(aabb, grid, 12, dev, shadingMode="MLP_Fea_late_view", fea_pe=0, **kw)
    focal = max(H, W) / 2.0 * 1.7320508
    c2w = torch.eye(3, 4, device=dev)
    rays = rodynrf.camera_rays(c2w[None], focal, H, W, ndc=True, near=1.0)
    N = rays.shape[0]
    ts = torch.zeros(N, device=dev)
    L = 1.0 - a.tau

    def planes():
        xyz, z, valid = rodynrf.sampleXYZ(dy, rays, S, ray_type=rt, is_train=False)
        o_s = st(rays, ts, None, xyz, z, valid, ray_type=rt, N_samples=S, rgb=False)
        o_d = dy(rays, ts, None, xyz, z, valid, ray_type=rt, N_samples=S, rgb=False)
        return z, o_s.sigma, o_d.sigma, o_d.blending, o_d.dists

    def leg_a():
        with torch.no_grad():
            maps = rodynrf.render_rays(st, dy, rays, ts, N_samples=S, ray_type=rt, maps=True)
            z, ss, sd, b, d = planes()
            a_d, a_s = 1.0 - torch.exp(-sd * d), 1.0 - torch.exp(-ss * d)
            T = torch.cumprod((1.0 - a_d * b) * (1.0 - a_s * (1.0 - b)) + 1e-10, -1)
            j = torch.searchsorted(-T, torch.full((N, 1), -L, device=dev)).clamp(max=S - 1)
            return maps, z.gather(1, j)[:, 0]

    def leg_b():
        return rodynrf.render_hits(st, dy, rays, ts, a.tau, N_samples=S, ray_type=rt, maps=True)

    def leg_c():
        return rodynrf.render_hits(st, dy, rays, ts, a.tau, N_samples=S, ray_type=rt)

    with torch.no_grad():
        z, ss, sd, b, _ = planes()

    def leg_k():
        return rodynrf.hits_from_planes(rays, z, ss, sd, b, tau=a.tau, ray_type=rt, distance_scale=dy.distance_scale)

    legs = {"a": leg_a, "b": leg_b, "c": leg_c, "k": leg_k}
    for _ in range(3):
        out = {n: f() for n, f in legs.items()}
    t = {n: [] for n in legs}
    for _ in range(a.rounds):
        for n, f in legs.items():
            t[n].append(timed(f))
    med = {n: statistics.median(v) for n, v in t.items()}
    hit = float(out["c"]["hit"].float().mean())
    gap = float((out["a"][1] - out["c"]["z"]).abs()[out["c"]["hit"]].max())
    lines = [f"frame {H} x {W} = {N} rays, grid {grid}, S = {S}, tau = {a.tau}, {a.rounds} interleaved rounds; hit share {hit:.3f}; "
             f"max |sample-resolution median depth of (a) - z_hit| {gap:.3e} (a sample step is {1.0 / (S - 1):.3e})"]
    names = {"a": "(a) render_rays(maps) + planes + cumprod + searchsorted", "b": "(b) render_hits(maps=True)",
             "c": "(c) render_hits(maps=False)", "k": "(k) k_render_hits alone (hits_from_planes)"}
    for n in legs:
        lines.append(f"{names[n]:58s} {med[n]:8.3f} ms [{min(t[n]):.3f}, {max(t[n]):.3f}]")
    lines.append(f"(a)/(b) x{med['a'] / med['b']:.2f}   (a)/(c) x{med['a'] / med['c']:.2f}   (c) - (b) {med['c'] - med['b']:+.3f} ms against the "
                 f"spread of (b) {max(t['b']) - min(t['b']):.3f} ms")
    lines.append(f"k_render_hits: {16.0 * N * S / (med['k'] * 1e-3) / 1e9:.1f} GB/s of the four [N][S] planes ({16 * S} bytes per ray)")
    for s in lines:
        print(s, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
