"""Time track_visibility (rdrf_track_visibility_fwd) against the composition of public calls that gives the same number
without it: the slots' rays in torch (generate_rays with the tracks' own pixels), sampleXYZ, two forward(rgb=False) calls
with all S samples, and a cumprod of the compositor's factor up to the point's depth.  M points, K slots, at the grid and
sample count of the first and the last stage of the Nvidia config (scene_config("nvidia"), resolution_stages).  Interleaved
rounds (native, composition, native, ...), HIP events around each leg on the current stream after a warm-up, medians and the
min-max spread.  Also prints the share of the M K S samples that lie in front of their point (valid and z < zq): the only
samples the native call evaluates.

    python tools/bench_track_vis.py [--M 4096] [--K 24] [--rounds 15] [--out FILE]"""
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
    ap.add_argument("--M", type=int, default=4096)
    ap.add_argument("--K", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import rodynrf
    from _gpu_util import COMMON
    dev = "cuda"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    torch.manual_seed(11)
    cfg = rodynrf.scene_config("nvidia")
    stages = rodynrf.resolution_stages(cfg)
    H, W, T, rt = cfg["H"], cfg["W"], 101, "ndc"
    M, K = a.M, a.K
    n_bwd = (K - 1) // 2
    n_fwd = K - 1 - n_bwd
    aabb = torch.tensor(cfg["aabb"])
    focal = max(H, W) / 2.0 * 1.7320508
    p9 = torch.zeros(K, 9)
    p9[:, 0] = 1
    p9[:, 4] = 1
    p9 = (p9 + 0.02 * torch.randn(K, 9)).to(dev)
    cams = rodynrf.pose_to_mtx(p9)
    for name, (_, grid, S) in (("stage 0", stages[0]), ("final stage", stages[-1])):
        # density_shift -2: a ray's optical depth is of order 5, as in tests/test_gpu_track_vis.py
        kw = dict(COMMON, near_far=[0.0, 1.0], density_shift=-2.0, fea2denseAct="softplus")
        st = rodynrf.TensorVMSplit(aabb, grid, 12, dev, shadingMode="MLP_Fea", fea_pe=2, **kw)
        dy = rodynrf.TensorVMSplit_TimeEmbedding(aabb, grid, 12, dev, shadingMode="MLP_Fea_late_view", fea_pe=0, **kw)
        # seeds: pixels of the middle camera at depths spread uniformly over the sampled range
        ids = torch.randint(0, H * W, (M,), device=dev) + n_bwd * H * W
        rays0 = rodynrf.generate_rays(ids, p9, focal, H, W, ndc=True, near=1.0)
        p0 = rays0[:, :3] + rays0[:, 3:] * torch.rand(M, 1, device=dev)
        t0 = torch.zeros(M, device=dev)
        tr = rodynrf.track_points(dy, p0, t0, n_fwd, n_bwd, T, cameras=cams, focal=focal, H=H, W=W, ray_type=rt)
        margin = 2.0 / (S - 1)
        view = (torch.arange(K, device=dev) * (H * W))[None].expand(M, K).reshape(-1)
        dt = 2.0 / (T - 1)
        ts = (t0[:, None] + dt * tr.frames_offset[None].float()).reshape(-1)
        zq = ((tr.points[..., 2].clamp(-1.0, 1.0 - 1e-6) + 1.0) / 2.0 - margin).reshape(-1)

        def native():
            return rodynrf.track_visibility(st, dy, tr, t0, n_fwd, n_bwd, T, cams, focal, H, W, N_samples=S, ray_type=rt, margin=margin)

        def compose(share=False):
            with torch.no_grad():
                rays = rodynrf.generate_rays(view, p9, focal, H, W, ndc=True, near=1.0, uv=tr.pixels.reshape(-1, 2))
                xyz, z, valid = rodynrf.sampleXYZ(dy, rays, S, ray_type=rt, is_train=False)
                o_s = st(rays, ts, None, xyz, z, valid, ray_type=rt, N_samples=S, rgb=False)
                o_d = dy(rays, ts, None, xyz, z, valid, ray_type=rt, N_samples=S, rgb=False)
                if share:
                    return float((valid & (z < zq[:, None])).float().mean())
                # the factor of every sample over its part in front of zq, then the product
                width = torch.cat([z[:, 1:] - z[:, :-1], torch.zeros_like(z[:, :1])], -1)
                frac = torch.where(width > 0, ((zq[:, None] - z) / width.clamp(min=1e-30)).clamp(0.0, 1.0), torch.zeros_like(z))
                d = o_d.dists * frac
                a_d, a_s, b = 1.0 - torch.exp(-o_d.sigma * d), 1.0 - torch.exp(-o_s.sigma * d), o_d.blending
                return torch.cumprod((1.0 - a_d * b) * (1.0 - a_s * (1.0 - b)) + 1e-10, -1)[:, -1].reshape(M, K)

        for _ in range(3):
            vn, vc = native(), compose()
        front = tr.pixels.isfinite().all(-1)
        diff = float((vn - vc)[front].abs().max())
        tn, tc = [], []
        for _ in range(a.rounds):
            tn.append(timed(native))
            tc.append(timed(compose))
        mn, mc = statistics.median(tn), statistics.median(tc)
        say(f"{name:11s} grid {grid} S={S:3d} M={M} K={K}  native {mn:8.3f} ms [{min(tn):.3f}, {max(tn):.3f}]  composition {mc:8.3f} ms "
            f"[{min(tc):.3f}, {max(tc):.3f}]  x{mc / mn:.2f}  samples in front of the points {compose(True):.3f}  "
            f"max |native - composition| {diff:.2e}  mean vis {float(vn.mean()):.3f}")
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
