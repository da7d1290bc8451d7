#!/usr/bin/env python
"""Time of the isosurface extraction (rdrf_iso_count + rdrf_iso_emit, device time between HIP events, median of --reps)
on a 200^3 ball and on the dense alpha volume of the nvidia final-stage grid, beside the getDenseAlpha call that feeds it.

The simplification leg (--simplify K, default 2; 0 skips it) clusters each of those meshes K lattice cells wide and times
rdrf_simplify_count + rdrf_simplify_emit the same way, beside the same clustering composed in torch on the device
(torch.unique(return_inverse) + index_add_ + a boolean face mask) and beside the rdrf_iso_emit that produced the input.

    python tools/bench_mesh.py [--reps 5] [--out FILE] [--simplify K] [--simplify-out FILE]"""
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
    return t_count, t_emit, nv, nf, (verts, faces, nrm)


def torch_clustering(verts, faces, normals, origin, cell, n):
    """the same clustering composed of torch ops (fp64 sums through index_add_, whose order is not fixed)"""
    c = torch.floor((verts - origin) / cell).clamp_(min=0)
    c = torch.minimum(c, (n - 1).to(c.dtype)).long()
    key = (c[:, 0] * n[1] + c[:, 1]) * n[2] + c[:, 2]
    uniq, cluster, k = torch.unique(key, return_inverse=True, return_counts=True)
    fc = cluster[faces.long()]
    keep = (fc[:, 0] != fc[:, 1]) & (fc[:, 1] != fc[:, 2]) & (fc[:, 0] != fc[:, 2])
    fc = fc[keep]
    used = torch.zeros(len(uniq), dtype=torch.bool, device=verts.device)
    used[fc.reshape(-1)] = True
    new = torch.cumsum(used, 0) - 1
    pos = torch.zeros(len(uniq), 3, dtype=torch.float64, device=verts.device).index_add_(0, cluster, verts.double())
    out = [(pos / k[:, None].double())[used].float(), new[fc].int()]
    if normals is not None:
        s = torch.zeros(len(uniq), 3, dtype=torch.float64, device=verts.device).index_add_(0, cluster, normals.double())
        out.append(torch.nn.functional.normalize(s[used], dim=1).float())
    return out


def simplification(mesh, box, shape, K, reps):
    """count and emit timed apart, as the extraction; -> (ms count, ms emit, ms torch, V', F', bytes the native path moves at least)"""
    import rodynrf
    L = rodynrf._lib
    verts, faces, nrm = mesh
    V, F = verts.shape[0], faces.shape[0]
    lat = rodynrf.simplify_lattice(box, shape, K)
    o3, c3, n3 = (C.c_float * 3)(*[float(v) for v in lat["aabb"][:3]]), (C.c_float * 3)(*lat["cell"]), (C.c_int * 3)(*lat["grid"])
    ws = L.workspace(verts.device, L.lib.rdrf_simplify_ws_bytes(V, F, n3))
    counts = torch.empty(2, dtype=torch.int64, device=verts.device)
    s = L.stream_of(verts)
    t_count, _ = timed(lambda: L.check(L.lib.rdrf_simplify_count(L.ptr(verts), V, L.ptr(faces), F, o3, c3, n3, 1, L.ptr(ws), ws.numel(),
                                                                 L.ptr(counts), None, s), "rdrf_simplify_count"), reps)
    nv, nf = counts.cpu().tolist()
    vo, fo = torch.empty(nv, 3, device=verts.device), torch.empty(nf, 3, dtype=torch.int32, device=verts.device)
    no = torch.empty(nv, 3, device=verts.device) if nrm is not None else None
    t_emit, _ = timed(lambda: L.check(L.lib.rdrf_simplify_emit(L.ptr(verts), L.ptr(nrm), None, V, L.ptr(faces), F, L.ptr(ws), L.ptr(vo), L.ptr(no),
                                                               None, L.ptr(fo), nv, nf, s), "rdrf_simplify_emit"), reps)
    dev = verts.device
    origin, cell = lat["aabb"][:3].to(dev), torch.tensor(lat["cell"], dtype=torch.float32, device=dev)
    n = torch.tensor(lat["grid"], device=dev)
    t_torch, ref = timed(lambda: torch_clustering(verts, faces, nrm, origin, cell, n), reps)
    assert ref[0].shape[0] == nv and torch.equal(ref[1], fo), "the torch composition disagrees with the native clustering"
    per_v = 12 * (2 if nrm is not None else 1)
    moved = V * per_v * 2 + F * 12 * 2 + nv * per_v + nf * 12   # inputs read by count (verts, faces) and by emit, outputs written
    return t_count, t_emit, t_torch, nv, nf, moved


def simplify_line(name, mesh, box, shape, K, reps, t_iso_emit):
    tc, te, tt, nv, nf, moved = simplification(mesh, box, shape, K, reps)
    V, F = mesh[0].shape[0], mesh[1].shape[0]
    return (f"{name} simplify K={K} normals={int(mesh[2] is not None)}: count {tc:.3f} ms + emit {te:.3f} ms = {tc + te:.3f} ms; torch composition "
            f"{tt:.3f} ms (native / torch = {(tc + te) / tt:.2f}); the rdrf_iso_emit that produced the input {t_iso_emit:.3f} ms  "
            f"({V} -> {nv} vertices, {F} -> {nf} faces; {moved / 1e6:.1f} MB of mesh read and written: {moved / (tc + te) / 1e6:.0f} GB/s)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--simplify", type=int, default=2)
    ap.add_argument("--simplify-out", default=None)
    a = ap.parse_args()
    import rodynrf
    from rodynrf import scene_config
    lines, slines = [], []
    g = torch.linspace(-1, 1, 200, device="cuda")
    x, y, z = torch.meshgrid(g, g, g, indexing="ij")
    ball = (0.7 - (x * x + y * y + z * z).sqrt()).contiguous()
    for normals in (False, True):
        tc, te, nv, nf, mesh = extraction(ball, 0.0, [-1, -1, -1, 1, 1, 1], normals, a.reps)
        if a.simplify > 0:
            slines.append(simplify_line("ball 200^3", mesh, [-1, -1, -1, 1, 1, 1], ball.shape, a.simplify, a.reps, te))
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
    tc, te, nv, nf, mesh = extraction(alpha, level, dy.aabb.cpu(), True, a.reps)
    if a.simplify > 0:
        slines.append(simplify_line(f"nvidia final grid {cfg['grid']}", mesh, dy.aabb.cpu(), alpha.shape, a.simplify, a.reps, te))
    lines.append(f"nvidia final grid {cfg['grid']} (dynamic field, one time): getDenseAlpha {t_alpha:.1f} ms; count {tc:.3f} ms + emit {te:.3f} ms "
                 f"= {tc + te:.3f} ms = {100 * (tc + te) / t_alpha:.1f} % of it  ({nv} vertices, {nf} faces at level {level:.3g}, normals on)")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    if slines:
        print("\n".join(slines))
        if a.simplify_out:
            with open(a.simplify_out, "w") as f:
                f.write("\n".join(slines) + "\n")


if __name__ == "__main__":
    main()
