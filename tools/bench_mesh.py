#!/usr/bin/env python
"""Time of the isosurface extraction (rdrf_iso_count + rdrf_iso_emit, device time between HIP events, median of --reps)
on a 200^3 ball and on the dense alpha volume of the nvidia final-stage grid, beside the getDenseAlpha call that feeds it.

    python tools/bench_mesh.py [--reps 5] [--out FILE]"""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


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


def extraction(vol, level, aabb, normals, reps):
    """count and emit timed apart (the host read of the counts sits between them and is not device time)"""
    import rodynrf
    L = rodynrf._lib
    G0, G1, G2 = vol.shape[:3]
    T = 1 if vol.dim() == 3 else vol.shape[3]
    ws = L.workspace(vol.device, L.lib.rdrf_iso_ws_bytes(G0, G1, G2))
    counts = torch.empty(2, dtype=torch.int64, device=vol.device)
    s = L.stream_of(vol)
    t_count, _ = timed(lambda: L.check(L.lib.rdrf_iso_count(L.ptr(vol), G0, G1, G2, T, 0, level, L.ptr(ws), ws.numel(), L.ptr(counts), s),
                                       "rdrf_iso_count"), reps)
    nv, nf = counts.cpu().tolist()
    verts, faces = torch.empty(nv, 3, device=vol.device), torch.empty(nf, 3, dtype=torch.int32, device=vol.device)
    nrm = torch.empty(nv, 3, device=vol.device) if normals else None
    box = (C.c_float * 6)(*[float(v) for v in torch.as_tensor(aabb).reshape(-1)])
    t_emit, _ = timed(lambda: L.check(L.lib.rdrf_iso_emit(L.ptr(vol), G0, G1, G2, T, 0, level, box, 0, L.ptr(ws), L.ptr(verts), L.ptr(nrm),
                                                          L.ptr(faces), nv, nf, s), "rdrf_iso_emit"), reps)
    return t_count, t_emit, nv, nf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import rodynrf
    from rodynrf import scene_config
    lines = []
    g = torch.linspace(-1, 1, 200, device="cuda")
    x, y, z = torch.meshgrid(g, g, g, indexing="ij")
    ball = (0.7 - (x * x + y * y + z * z).sqrt()).contiguous()
    for normals in (False, True):
        tc, te, nv, nf = extraction(ball, 0.0, [-1, -1, -1, 1, 1, 1], normals, a.reps)
        lines.append(f"ball 200^3 normals={int(normals)}: count {tc:.3f} ms + emit {te:.3f} ms = {tc + te:.3f} ms  ({nv} vertices, {nf} faces; "
                     f"the count pass reads 32 MB once: {0.032 / tc * 1e3:.0f} GB/s of volume)")
    cfg = scene_config("nvidia", "final")
    torch.manual_seed(0)
    kw = dict(density_n_comp=[16, 4, 4], appearance_n_comp=[48, 12, 12], app_dim=27, near_far=cfg["near_far"], alphaMask_thres=1e-4,
              density_shift=-10, distance_scale=25, pos_pe=6, view_pe=0, featureC=128, step_ratio=2.0, fea2denseAct="relu")
    dy = rodynrf.TensorVMSplit_TimeEmbedding(torch.tensor(cfg["aabb"]), cfg["grid"], cfg["T"], "cuda", shadingMode="MLP_Fea_late_view",
                                             fea_pe=0, **kw)
    t_alpha, (alpha, _) = timed(lambda: dy.getDenseAlpha(times=[0.0]), 2)
    level = float(alpha.float().mean())   # an untrained field: the mean puts a surface through the noise, far denser than a trained scene's
    tc, te, nv, nf = extraction(alpha, level, dy.aabb.cpu(), True, a.reps)
    lines.append(f"nvidia final grid {cfg['grid']} (dynamic field, one time): getDenseAlpha {t_alpha:.1f} ms; count {tc:.3f} ms + emit {te:.3f} ms "
                 f"= {tc + te:.3f} ms = {100 * (tc + te) / t_alpha:.1f} % of it  ({nv} vertices, {nf} faces at level {level:.3g}, normals on)")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
