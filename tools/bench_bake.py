#!/usr/bin/env python
"""Time of the native texture bake (mesh.bake_texture, csrc/rdrf_bake.hip) against the same bake composed of torch ops -- index
gathers for the corners, broadcasting for the weights, query_points (scene: scene_alpha_volume and both fields), the torch pack
-- on the 200^3 ball at simplify=2, q = 4, 8, 16, for the one-field bake and the scene bake.  Device time between HIP events
around the whole call, one warm-up of every shape, the two paths alternating rep by rep; median and spread of --reps.  The
field evaluation is common to both sides, so the gain is bounded by the share of the geometry and pack stages: the library's
timing hook gives that share.  Untrained fields (seed 0): the kernels' time does not depend on the weights.

Beside it the number that justifies the feature: the colour error of the textured K = 2 mesh (bilinear fetch) and of its
vertex-coloured twin (barycentric interpolation of the cluster means) against query_points at seeded surface points.

    python tools/bench_bake.py [--reps 5] [--out FILE]"""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

KERNELS = ("bake_fill", "bake_texels", "bake_pack", "point_static", "point_static_app", "time_branch", "point_dyn", "point_dyn_app",
           "point_prep", "scene_static", "scene_alpha")
VIEW, T = (0.0, 0.6, 0.8), 0.25


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def kernel_ms(L, fn):
    L.lib.rdrf_prof_reset()
    L.lib.rdrf_prof_enable(1)
    fn()
    torch.cuda.synchronize()
    out = {}
    for k in KERNELS:
        ms, n = C.c_double(0), C.c_int(0)
        L.lib.rdrf_prof_get(k.encode(), C.byref(ms), C.byref(n))
        if n.value:
            out[k] = ms.value
    L.lib.rdrf_prof_enable(0)
    L.lib.rdrf_prof_reset()
    return out


def quantise(rgb):
    return torch.round(rgb.clamp(0.0, 1.0) * 255.0).to(torch.uint8)


def composed(M, A, field, verts, faces, q, static=None):
    """the bake a caller could write with torch and the public point queries"""
    F, dev = faces.shape[0], verts.device
    Wt, Ht, R = M.atlas_layout(F, q)
    y, x = torch.meshgrid(torch.arange(Ht, device=dev), torch.arange(Wt, device=dev), indexing="ij")
    i, j = x % q, y % q
    upper = i + j > q - 1
    f = 2 * ((y // q) * R + x // q) + upper
    owned = (x < R * q) & (f < F)
    fv = faces[torch.where(owned, f, 0)].long()
    d = torch.where(upper, q - 3, q - 2).float()
    w1 = torch.where(upper, q - 1 - i, i).float() / d
    w2 = torch.where(upper, q - 1 - j, j).float() / d
    w0 = 1.0 - w1 - w2
    p = w0[..., None] * verts[fv[..., 0]] + w1[..., None] * verts[fv[..., 1]] + w2[..., None] * verts[fv[..., 2]]
    if static is None:
        rgb = field.query_points(p, T if field.DYNAMIC else None, VIEW, want=("rgb",))["rgb"]
    else:
        o = A.scene_alpha_volume(static, field, p.reshape(-1, 3), [T], want=("owner",))["owner"].view(Ht, Wt, 1)
        rgb = o * field.query_points(p, T, VIEW, want=("rgb",))["rgb"] + (1.0 - o) * static.query_points(p, None, VIEW, want=("rgb",))["rgb"]
    return torch.where(owned[..., None], quantise(rgb), torch.zeros(3, dtype=torch.uint8, device=dev))


def bilinear(tex, px, py):
    t = tex.float()
    fx, fy = px - 0.5, py - 0.5
    x0, y0 = fx.floor().long(), fy.floor().long()
    ax, ay = (fx - x0)[:, None], (fy - y0)[:, None]
    cx, cy = (lambda v: v.clamp(0, t.shape[1] - 1)), (lambda v: v.clamp(0, t.shape[0] - 1))
    return ((1 - ay) * ((1 - ax) * t[cy(y0), cx(x0)] + ax * t[cy(y0), cx(x0 + 1)])
            + ay * ((1 - ax) * t[cy(y0 + 1), cx(x0)] + ax * t[cy(y0 + 1), cx(x0 + 1)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import rodynrf
    from rodynrf import scene_config
    M, A, L = rodynrf.mesh, rodynrf.alpha, rodynrf._lib
    cfg = scene_config("nvidia", "final")
    torch.manual_seed(0)
    kw = dict(density_n_comp=[16, 4, 4], appearance_n_comp=[48, 12, 12], app_dim=27, near_far=cfg["near_far"], alphaMask_thres=1e-4,
              density_shift=0.0, distance_scale=25, pos_pe=6, view_pe=0, featureC=128, step_ratio=2.0, fea2denseAct="softplus")
    aabb = torch.tensor(cfg["aabb"])
    st = rodynrf.TensorVMSplit(aabb, cfg["grid"], cfg["T"], "cuda", shadingMode=cfg.get("static_head", "MLP_Fea"), fea_pe=2, **kw)
    dy = rodynrf.TensorVMSplit_TimeEmbedding(aabb, cfg["grid"], cfg["T"], "cuda", shadingMode="MLP_Fea_late_view", fea_pe=0, **kw)
    # the 200^3 ball in the field's box, meshed and clustered two cells wide
    G = 200
    box = aabb.reshape(2, 3).cuda()
    axes = [torch.linspace(float(box[0, d]), float(box[1, d]), G, device="cuda") for d in range(3)]
    X, Y, Z = torch.meshgrid(*axes, indexing="ij")
    half = (box[1] - box[0]) / 2
    centre = (box[0] + box[1]) / 2
    vol = 0.8 - torch.sqrt(((X - centre[0]) / half[0]) ** 2 + ((Y - centre[1]) / half[1]) ** 2 + ((Z - centre[2]) / half[2]) ** 2)
    fine_v, fine_f = rodynrf.extract_isosurface(vol, 0.0, aabb)
    lattice = rodynrf.simplify_lattice(aabb, vol.shape, 2)
    fine_c = rodynrf.vertex_colors(dy, fine_v, T, VIEW)
    verts, faces, vcol = rodynrf.simplify_mesh(fine_v, fine_f, lattice["cell"], lattice["grid"], lattice["aabb"], colors=fine_c)
    del vol, X, Y, Z
    F = faces.shape[0]
    lines = [f"{G}^3 ball: {fine_v.shape[0]} vertices, simplify=2: {verts.shape[0]} vertices, {F} faces; nvidia final untrained softplus "
             f"fields; ms per call, median (min .. max) of {a.reps} alternating reps"]
    for static in (None, st):
        for q in (4, 8, 16):
            native = lambda: M.bake_texture(dy, verts, faces, T, q, view=VIEW, static=static)[0]
            torchy = lambda: composed(M, A, dy, verts, faces, q, static)
            tn, tt = native(), torchy()   # the warm-up of both paths at this shape
            torch.cuda.synchronize()
            differ = int((tn != tt).any(-1).sum())
            ms = {"native": [], "torch": []}
            for _ in range(a.reps):
                for key, fn in (("native", native), ("torch", torchy)):
                    t, out = event_ms(fn)
                    del out
                    ms[key].append(t)
            med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
            show = lambda k: f"{med[k]:8.2f} ({min(ms[k]):.2f} .. {max(ms[k]):.2f})"
            ks = kernel_ms(L, native)
            own = sum(v for k, v in ks.items() if k.startswith("bake_"))
            total = sum(ks.values())
            lines.append(f"{'scene' if static is not None else 'field'} bake, q = {q:2d}, atlas {tn.shape[1]} x {tn.shape[0]}: native {show('native')}  "
                         f"torch ops {show('torch')}  ratio {med['torch'] / med['native']:.2f}x  texels that differ {differ} of {tn.shape[0] * tn.shape[1]}")
            lines.append(f"    native kernels: geometry + pack {own:.3f} ms of {total:.3f} ms ({100 * own / max(total, 1e-9):.1f} %): "
                         + ", ".join(f"{k} {v:.3f}" for k, v in ks.items()))
            del tn, tt
    # colour error at seeded surface points of the K = 2 mesh: texture against vertex colours
    g = torch.Generator(device="cuda").manual_seed(1)
    n = 200000
    fi = torch.randint(0, F, (n,), generator=g, device="cuda")
    r = torch.rand(n, 2, generator=g, device="cuda")
    flip = r.sum(-1) > 1
    r = torch.where(flip[:, None], 1 - r, r)
    w = torch.stack((1 - r.sum(-1), r[:, 0], r[:, 1]), -1)
    fv = faces[fi].long()
    pts = (w[..., None] * verts[fv]).sum(1)
    truth = dy.query_points(pts, T, VIEW, want=("rgb",))["rgb"].clamp(0, 1) * 255.0
    by_vertex = (w[..., None] * vcol[fv].float()).sum(1)
    lines.append(f"colour error against query_points at {n} seeded surface points of the K = 2 mesh, 8-bit levels, mean / 99th percentile / max:")
    stat = lambda e: f"{float(e.mean()):.3f} / {float(e.flatten().kthvalue(int(e.numel() * 0.99)).values):.3f} / {float(e.max()):.3f}"
    lines.append(f"    vertex colours (cluster means, barycentric): {stat((by_vertex - truth).abs())}")
    for q in (4, 8, 16):
        tex, uv = M.bake_texture(dy, verts, faces, T, q, view=VIEW)
        p = (w[..., None] * uv[fi]).sum(1) * torch.tensor([tex.shape[1], tex.shape[0]], device="cuda")
        lines.append(f"    texture, q = {q:2d} (bilinear fetch):               {stat((bilinear(tex, p[:, 0], p[:, 1]) - truth).abs())}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
