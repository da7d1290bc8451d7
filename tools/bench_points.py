#!/usr/bin/env python
"""Time of the point queries (TensorBase.query_points, csrc/rdrf_point.hip) on the nvidia final-stage grid: device time between
HIP events around the whole call (allocations and launches included), one warm-up, median of --reps, for both fields, with and
without rgb, one shared time; beside it compute_alpha at the same M with one time (the density side's neighbour), the per-kernel
times of the library's timing hook, and the per-sample time of the forward appearance kernels on a ray batch of the same fields
(what bench.py --full's kernel table divides out).  Then the colours of a mesh: vertex_colors on the vertices of the 200^3 ball
of tools/bench_mesh.py, and colored_mesh against field_mesh on a 200^3 lattice of the dynamic field.

    python tools/bench_points.py [--reps 7] [--out FILE]"""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

KERNELS = ("time_branch", "point_dyn", "point_static", "point_prep", "point_dyn_app", "point_static_app")


def timed(fn, reps):
    ms = []
    for _ in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return sorted(ms[1:])[len(ms[1:]) // 2], out


def kernel_ms(L, fn, names):
    """{name: ms per launch} of one call of fn under the library's timing hook"""
    fn()
    torch.cuda.synchronize()
    L.lib.rdrf_prof_reset()
    L.lib.rdrf_prof_enable(1)
    fn()
    torch.cuda.synchronize()
    out = {}
    for k in names:
        ms, n = C.c_double(0), C.c_int(0)
        L.lib.rdrf_prof_get(k.encode(), C.byref(ms), C.byref(n))
        if n.value:
            out[k] = ms.value / n.value
    L.lib.rdrf_prof_enable(0)
    L.lib.rdrf_prof_reset()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import rodynrf
    from rodynrf import scene_config
    alpha_volume = rodynrf.alpha.alpha_volume
    L = rodynrf._lib
    cfg = scene_config("nvidia", "final")
    torch.manual_seed(0)
    kw = dict(density_n_comp=[16, 4, 4], appearance_n_comp=[48, 12, 12], app_dim=27, near_far=cfg["near_far"], alphaMask_thres=1e-4,
              density_shift=-10, distance_scale=25, pos_pe=6, view_pe=0, featureC=128, step_ratio=2.0, fea2denseAct="relu")
    aabb = torch.tensor(cfg["aabb"])
    st = rodynrf.TensorVMSplit(aabb, cfg["grid"], cfg["T"], "cuda", shadingMode=cfg.get("static_head", "MLP_Fea"), fea_pe=2, **kw)
    dy = rodynrf.TensorVMSplit_TimeEmbedding(aabb, cfg["grid"], cfg["T"], "cuda", shadingMode="MLP_Fea_late_view", fea_pe=0, **kw)
    fields = (("static", st, ("sigma", "rgb")), ("dynamic", dy, ("sigma", "rgb", "blending", "xyz_prime")))
    lines = [f"nvidia final grid {cfg['grid']}, untrained fields, one shared time; ms per call (ns per point)"]
    box = dy.aabb
    for M in (4096, 65536, 1048576):
        pts = (box[0] + torch.rand(M, 3, device="cuda") * (box[1] - box[0])).contiguous()
        vd = torch.nn.functional.normalize(torch.randn(M, 3, device="cuda"), dim=-1).contiguous()
        tone = torch.tensor([0.25], device="cuda")
        for name, f, outs in fields:
            no_rgb = tuple(o for o in outs if o != "rgb")
            t_all, _ = timed(lambda: f.query_points(pts, 0.25, vd, want=outs), a.reps)
            t_den, _ = timed(lambda: f.query_points(pts, 0.25, want=no_rgb), a.reps)
            t_alpha, _ = timed(lambda: alpha_volume(f, pts, tone, 1.0), a.reps)
            ks = kernel_ms(L, lambda: f.query_points(pts, 0.25, vd, want=outs), KERNELS)
            per = lambda ms: f"{ms:.3f} ({ms * 1e6 / M:.2f})"
            lines.append(f"M={M:8d} {name:7s}: with rgb {per(t_all)}  without rgb {per(t_den)}  compute_alpha {per(t_alpha)}  kernels: "
                         + ", ".join(f"{k} {per(v)}" for k, v in ks.items()))
    # the forward appearance kernels on a ray batch of the same fields: ms per app-masked sample
    N, S = 4096, cfg.get("n_samples", 256)
    rays = torch.cat([torch.stack([torch.empty(N).uniform_(-1.4, 1.4), torch.empty(N).uniform_(-1.5, 1.5), -torch.ones(N)], -1),
                      torch.stack([torch.randn(N) * 0.1, torch.randn(N) * 0.1, 2 * torch.ones(N)], -1)], -1).cuda()
    ts = (torch.randint(0, 12, (N,)).float() * 2 / 11 - 1).cuda()
    with torch.no_grad():
        xyz, z, valid = rodynrf.sampleXYZ(dy, rays, S, ray_type="ndc", is_train=False)
        for name, f, _ in fields:
            fwd = lambda: f(rays, ts, None, xyz, z, valid, ray_type="ndc")
            o = fwd()
            masked = int((o.weight > f.rayMarch_weight_thres).sum())
            key = "static_app" if name == "static" else "dyn_app"
            ks = kernel_ms(L, fwd, (key, "dyn_density", "static_density"))
            dens = ks.get("dyn_density", ks.get("static_density", 0.0))
            lines.append(f"forward {name:7s} N={N} S={S}: {key} {ks.get(key, 0.0):.3f} ms for {masked} app-masked samples = "
                         f"{ks.get(key, 0.0) * 1e6 / max(masked, 1):.2f} ns per sample; density kernel {dens:.3f} ms = "
                         f"{dens * 1e6 / (N * S):.2f} ns per sample")
    # colours of a mesh
    g = torch.linspace(-1, 1, 200, device="cuda")
    x, y, zz = torch.meshgrid(g, g, g, indexing="ij")
    ball = (0.7 - (x * x + y * y + zz * zz).sqrt()).contiguous()
    t_mesh, (verts, faces) = timed(lambda: rodynrf.extract_isosurface(ball, 0.0, dy.aabb), a.reps)
    for name, f, _ in fields:
        t_col, _ = timed(lambda: rodynrf.vertex_colors(f, verts, 0.25), a.reps)
        lines.append(f"ball 200^3 in the field's box: extract_isosurface {t_mesh:.3f} ms ({verts.shape[0]} vertices); vertex_colors {name} "
                     f"{t_col:.3f} ms = {t_col * 1e6 / verts.shape[0]:.2f} ns per vertex")
    alpha, _ = dy.getDenseAlpha((200, 200, 200), times=[0.25])
    level = float(alpha.mean())
    del alpha
    t_plain, plain = timed(lambda: rodynrf.field_mesh(dy, 0.25, level, (200, 200, 200)), 3)
    t_color, _ = timed(lambda: rodynrf.colored_mesh(dy, 0.25, level, (200, 200, 200)), 3)
    lines.append(f"dynamic field, 200^3 lattice, level {level:.3g} (untrained: a surface through noise, {plain[0].shape[0]} vertices): "
                 f"field_mesh {t_plain:.1f} ms, colored_mesh {t_color:.1f} ms (+{t_color - t_plain:.1f} ms = "
                 f"{(t_color - t_plain) * 1e6 / max(plain[0].shape[0], 1):.2f} ns per vertex)")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
