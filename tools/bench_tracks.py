"""Time track_points (one native launch) against the composition of public calls it replaces (one scene-flow launch, an add
and a clamp per step, one projection launch per slot): M points, K = n_bwd + 1 + n_fwd slots, both ray types, with and
without the projection.  Interleaved rounds (native, composition, native, ...), wall time around a device synchronise,
medians and the min-max spread.  Also times render_rays on a fixed chunk, for a same-kernels check between commits.

    python tools/bench_tracks.py [--M 4096] [--rounds 15] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default=None)
    ap.add_argument("--render-only", action="store_true", help="only the render_rays timing (RDRF_LIB selects the library)")
    a = ap.parse_args()
    import rodynrf
    from _gpu_util import COMMON, make_rays
    dev = "cuda"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    torch.manual_seed(7)
    T, H, W = 101, 270, 480
    for rt in (() if a.render_only else ("ndc", "contract")):
        aabb = torch.tensor([[-1.5, -1.67, -1.0], [1.5, 1.67, 1.0]]) if rt == "ndc" else torch.tensor([[-2.0] * 3, [2.0] * 3])
        kw = dict(COMMON, near_far=[0.0, 1.0] if rt == "ndc" else [0.0, 256.0], density_shift=-10.0, fea2denseAct="relu")
        dy = rodynrf.TensorVMSplit_TimeEmbedding(aabb, [48, 52, 32], 12, dev, shadingMode="MLP_Fea_late_view", fea_pe=0, **kw)
        lo, hi = aabb
        p0 = (lo + (hi - lo) * torch.rand(a.M, 3)).to(dev) * 0.9
        t0 = torch.zeros(a.M, device=dev)
        for K in (25, 100):
            n_bwd = (K - 1) // 2
            n_fwd = K - 1 - n_bwd
            p9 = torch.zeros(K, 9)
            p9[:, 0] = 1
            p9[:, 4] = 1
            cams = rodynrf.pose_to_mtx(p9 + 0.02 * torch.randn(K, 9)).to(dev)
            focal = 400.0
            dt = 2.0 / (T - 1)

            def compose(project):
                with torch.no_grad():
                    pts = [None] * K
                    pts[n_bwd] = p0
                    for d, n in ((0, n_fwd), (1, n_bwd)):
                        p, t = p0, t0
                        for k in range(1, n + 1):
                            p = p + dy.get_forward_backward_scene_flow(p.reshape(-1, 1, 3), t)[d].reshape(-1, 3)
                            if rt == "contract":
                                p = torch.clamp(p, min=-2.0 + 1e-6, max=2.0 - 1e-6)
                            t = t + dt if d == 0 else t - dt
                            pts[n_bwd + k if d == 0 else n_bwd - k] = p
                    out = [torch.stack(pts, 1)]
                    if project:
                        one, zero = torch.ones(a.M, 1, device=dev), torch.zeros(a.M, 6, device=dev)
                        for k in range(K):
                            c2w = cams[k][None].expand(a.M, 3, 4)
                            if rt == "ndc":
                                out.append(rodynrf.render_single_3d_point(H, W, focal, c2w, pts[k]))
                            else:
                                out.append(rodynrf.render_3d_point(H, W, focal, c2w, one, pts[k].reshape(-1, 1, 3), zero, rt))
                    return out

            def native(project):
                if project:
                    return rodynrf.track_points(dy, p0, t0, n_fwd, n_bwd, T, cameras=cams, focal=focal, H=H, W=W, ray_type=rt)
                return rodynrf.track_points(dy, p0, t0, n_fwd, n_bwd, T, ray_type=rt)

            for project in (False, True):
                for _ in range(2):
                    native(project)
                    compose(project)
                tn, tc = [], []
                for _ in range(a.rounds):
                    tn.append(timed(lambda: native(project)))
                    tc.append(timed(lambda: compose(project)))
                mn, mc = statistics.median(tn), statistics.median(tc)
                say(f"{rt:8s} M={a.M} K={K:3d} projection={int(project)}  native {mn:8.3f} ms [{min(tn):.3f}, {max(tn):.3f}]  "
                    f"composition {mc:8.3f} ms [{min(tc):.3f}, {max(tc):.3f}]  x{mc / mn:.1f}  per step native {1e3 * mn / (K - 1):.1f} us")
    # render_rays on a fixed chunk (the same kernels before and after this feature)
    aabb = torch.tensor([[-1.5, -1.67, -1.0], [1.5, 1.67, 1.0]])
    kw = dict(COMMON, near_far=[0.0, 1.0], density_shift=-10.0, fea2denseAct="relu")
    st = rodynrf.TensorVMSplit(aabb, [48, 52, 32], 12, dev, shadingMode="MLP_Fea", fea_pe=2, **kw)
    dy = rodynrf.TensorVMSplit_TimeEmbedding(aabb, [48, 52, 32], 12, dev, shadingMode="MLP_Fea_late_view", fea_pe=0, **kw)
    rays, ts = make_rays(8192, 1)
    rays, ts = rays.to(dev), ts.to(dev)
    for _ in range(3):
        rodynrf.render_rays(st, dy, rays, ts, 115)
    tr = [timed(lambda: rodynrf.render_rays(st, dy, rays, ts, 115)) for _ in range(a.rounds)]
    say(f"render_rays N=8192 S=115  {statistics.median(tr):.3f} ms [{min(tr):.3f}, {max(tr):.3f}]")
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
