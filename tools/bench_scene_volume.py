#!/usr/bin/env python
"""Time of the whole-scene alpha volume (alpha.scene_dense_alpha, csrc/rdrf_scene_alpha.hip) against the same volume composed
from the public calls that were there before it -- query_points on both fields in chunks, a call per time, plus the torch
expression 1 - (1 - a_d b)(1 - a_s (1 - b)) -- on the nvidia final-stage lattice with T = 1 and T = 12 and on 200^3.  Device
time between HIP events around the whole call (lattice, allocations and launches included), one warm-up of every shape, the
two paths alternating rep by rep; median and spread (min .. max) of --reps.  Beside it the largest difference between the two
volumes, the bytes each path writes, and the per-kernel times of the library's timing hook.  Untrained fields (seed 0): the
kernels' time does not depend on the weights.

    python tools/bench_scene_volume.py [--reps 5] [--out FILE]"""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

KERNELS = ("scene_static", "time_branch", "scene_alpha", "point_static", "point_dyn", "alpha_dyn")
TORCH_TEMPS = 11   # [M] tensors the composed path's torch expression writes per time: -s l, exp, 1 - e (a_d); a_d b, 1 - ., 1 - b,
#                    a_s (1 - b), 1 - ., the product, 1 - ., the copy into the volume's column


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def kernel_ms(L, fn, names):
    """{name: (ms in all launches, launches)} of one call of fn under the library's timing hook"""
    L.lib.rdrf_prof_reset()
    L.lib.rdrf_prof_enable(1)
    fn()
    torch.cuda.synchronize()
    out = {}
    for k in names:
        ms, n = C.c_double(0), C.c_int(0)
        L.lib.rdrf_prof_get(k.encode(), C.byref(ms), C.byref(n))
        if n.value:
            out[k] = (ms.value, n.value)
    L.lib.rdrf_prof_enable(0)
    L.lib.rdrf_prof_reset()
    return out


def composed(A, st, dy, gs, times):
    """what a caller could do before scene_dense_alpha: the lattice, the static sigma once, per time the dynamic field's sigma
    and blending, the expression in torch"""
    _, tt, dense, _ = A._dense_lattice(dy, gs, times)
    pts = dense.reshape(-1, 3)
    length = dy._step_host
    alpha = torch.empty(pts.shape[0], tt.numel(), device=pts.device)
    a_s = 1.0 - torch.exp(-st.query_points(pts, want=("sigma",))["sigma"] * length)
    for k, t in enumerate(tt.cpu().tolist()):
        q = dy.query_points(pts, t, want=("sigma", "blending"))
        a_d, b = 1.0 - torch.exp(-q["sigma"] * length), q["blending"]
        alpha[:, k] = 1.0 - (1.0 - a_d * b) * (1.0 - a_s * (1.0 - b))
    return alpha.view(*gs, tt.numel())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import rodynrf
    from rodynrf import scene_config
    A, L = rodynrf.alpha, rodynrf._lib
    cfg = scene_config("nvidia", "final")
    torch.manual_seed(0)
    kw = dict(density_n_comp=[16, 4, 4], appearance_n_comp=[48, 12, 12], app_dim=27, near_far=cfg["near_far"], alphaMask_thres=1e-4,
              density_shift=0.0, distance_scale=25, pos_pe=6, view_pe=0, featureC=128, step_ratio=2.0, fea2denseAct="softplus")
    aabb = torch.tensor(cfg["aabb"])
    st = rodynrf.TensorVMSplit(aabb, cfg["grid"], cfg["T"], "cuda", shadingMode=cfg.get("static_head", "MLP_Fea"), fea_pe=2, **kw)
    dy = rodynrf.TensorVMSplit_TimeEmbedding(aabb, cfg["grid"], cfg["T"], "cuda", shadingMode="MLP_Fea_late_view", fea_pe=0, **kw)
    lines = [f"nvidia final grid {cfg['grid']}, untrained softplus fields; ms per call, median (min .. max) of {a.reps} alternating reps"]
    all_times = A.lattice_times(cfg["T"]).tolist()
    for gs, times in ((list(cfg["grid"]), [0.25]), (list(cfg["grid"]), all_times), ([200, 200, 200], [0.25]), ([200, 200, 200], all_times)):
        M, Tn = gs[0] * gs[1] * gs[2], len(times)
        native = lambda: rodynrf.scene_dense_alpha(st, dy, gs, times)[0]
        public = lambda: composed(A, st, dy, gs, times)
        dyn_only = lambda: dy.getDenseAlpha(gs, times)[0]
        vn, vp = native(), public()   # the warm-up of both paths at this shape
        dyn_only()
        torch.cuda.synchronize()
        diff = float((vn - vp).abs().max())
        del vn, vp
        ms = {"native": [], "public": [], "dyn": []}
        for _ in range(a.reps):
            for key, fn in (("native", native), ("public", public), ("dyn", dyn_only)):
                t, out = event_ms(fn)
                del out
                ms[key].append(t)
        med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
        show = lambda k: f"{med[k]:9.2f} ({min(ms[k]):.2f} .. {max(ms[k]):.2f})"
        slabs = len(A._dense_lattice(dy, gs, times)[3])
        w_native = M * Tn * 4 + M * 4            # the volume + the static sigma of the pre-pass (workspace)
        w_public = M * 4 * 2 + Tn * M * 4 * (2 + TORCH_TEMPS) + M * Tn * 4   # sigma_s, a_s's temporaries; per time sigma_d, blending, the temporaries
        lines.append(f"lattice {gs[0]}x{gs[1]}x{gs[2]} = {M} points, T = {Tn:2d} ({slabs} slabs): scene_dense_alpha {show('native')}  "
                     f"composed from query_points + torch {show('public')}  ratio {med['public'] / med['native']:.2f}x  "
                     f"[getDenseAlpha of the dynamic field alone {show('dyn')}]  max |difference| {diff:.2e}  "
                     f"bytes written: native {w_native / 1e6:.0f} MB, composed {w_public / 1e6:.0f} MB (lattice points not counted: both write them)")
        ks = kernel_ms(L, native, KERNELS)
        kp = kernel_ms(L, public, KERNELS)
        fmt = lambda d: ", ".join(f"{k} {v[0]:.2f} ms / {v[1]} launches" for k, v in d.items())
        lines.append(f"    kernels, native: {fmt(ks)};  composed: {fmt(kp)}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
