"""Reconstruct a video from arrays:   python tools/fit_scene.py scene.npz out_dir [--config davis] [--iters N] [--graph]

scene.npz holds the arguments of rodynrf.Scene under their own names (rgb [T,H,W,3] uint8 | float32, flow_f / flow_b
[T,H,W,2], flow_mask_f / flow_mask_b [T,H,W], optionally disp, fg_mask, poses [T,3,4], focal, and held-out views as
heldout_c2w [K,3,4], heldout_t [K], heldout_rgb [K,H,W,3]).  The run follows the config's resolution schedule
(rodynrf.resolution_stages) and writes out_dir/run.th, run_static.th (the reference's checkpoint format), run_state.th (what
Trainer.load needs to continue the run) and metrics.json (PSNR / SSIM of the training frames and of the held-out views).
--resume continues from out_dir/run_state.th.  --alpha-mask G0,G1,G2: after the fit, updateAlphaMask on both fields at that
lattice and a second evaluation through the masked render; metrics.json then also holds "alpha_mask" (the occupied
fractions) and "train_masked" / "heldout_masked".  --tracks N: after the fit, the point tracks of N grid-spaced pixels of
the middle frame through the whole video (rodynrf.render_tracks) as out_dir/tracks.npz: points [N,T,3], pixels [N,T,2],
disp [N,T], acc_d [N] (weight of the dynamic field at the seed), query [N,2] (column, row), frame."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rodynrf  # noqa: E402


def track_queries(n, H, W):
    """n grid-spaced query pixels of an H x W image, [n,2] integer (column, row): the centres of the cells of a
    rows x cols lattice with cols / rows ~ W / H and rows * cols >= n, row-major, cut to n"""
    n = max(1, min(int(n), H * W))
    cols = max(1, min(W, round((n * W / H) ** 0.5)))
    rows = min(H, -(-n // cols))
    cols = min(W, -(-n // rows))      # (rows was capped by H: widen)
    ys = ((torch.arange(rows) + 0.5) * H / rows).long()
    xs = ((torch.arange(cols) + 0.5) * W / cols).long()
    return torch.stack(torch.meshgrid(xs, ys, indexing="xy"), -1).reshape(-1, 2)[:n]


def summary(metrics):
    """the line printed at the end: evaluation entries (those that carry psnr_mean) cut to their two means, the loss
    curve dropped, everything else as it is"""
    return {k: ({"psnr_mean": v["psnr_mean"], "ssim_mean": v["ssim_mean"]} if isinstance(v, dict) and "psnr_mean" in v else v)
            for k, v in metrics.items() if k != "loss"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("npz")
    ap.add_argument("out")
    ap.add_argument("--config", default=None, help="nvidia | nvidia_no_poses | davis (default: nvidia with poses, else nvidia_no_poses)")
    ap.add_argument("--iters", type=int, default=None, help="iterations of this call (default: to the config's n_iters)")
    ap.add_argument("--batch-size", type=int, default=None)
    ap.add_argument("--graph", action="store_true", help="replay captured iterations (single GPU)")
    ap.add_argument("--resume", action="store_true")
    ap.add_argument("--seed", type=int, default=20211202)
    ap.add_argument("--log-every", type=int, default=1000)
    ap.add_argument("--alpha-mask", default=None, metavar="G0,G1,G2",
                    help="build both fields' alpha masks on this lattice after the fit and evaluate with and without them")
    ap.add_argument("--tracks", type=int, default=0, metavar="N",
                    help="write tracks.npz: point tracks of N grid-spaced pixels of the middle frame (drawing is the caller's)")
    a = ap.parse_args()
    mask_grid = None
    if a.alpha_mask:
        mask_grid = [int(v) for v in a.alpha_mask.split(",")]
        if len(mask_grid) != 3 or min(mask_grid) < 1:
            ap.error("--alpha-mask takes three positive lattice sizes: G0,G1,G2")
    dev = torch.device("cuda", 0)
    scene = rodynrf.Scene.from_npz(a.npz, device=dev, seed=a.seed)
    cfg = rodynrf.scene_config(a.config or ("nvidia" if scene.has_poses else "nvidia_no_poses"))
    for k in ("T", "H", "W", "grid", "n_samples"):    # the scene's shape, the schedule's first grid
        cfg.pop(k, None)
    if a.batch_size:
        cfg["batch_size"] = a.batch_size
    tr = rodynrf.Trainer(cfg, dev, graph=a.graph, data=scene)
    os.makedirs(a.out, exist_ok=True)
    prefix = os.path.join(a.out, "run")
    if a.resume:
        tr.load(prefix)
    log = []

    def callback(trainer, it, loss):
        if it % a.log_every == 0:
            log.append((it, loss))     # device tensors: read once, at the end

    tr.fit(n_iters=a.iters, callback=callback)
    tr.save(prefix)
    metrics = dict(iterations=tr.it, grid=tr.cfg["grid"], n_samples=tr.cfg["n_samples"],
                   loss=[(it, float(l)) for it, l in log], train=rodynrf.evaluate(tr, scene, frames="train"))
    if scene.heldout:
        metrics["heldout"] = rodynrf.evaluate(tr, scene, frames="heldout")
    if mask_grid is not None:
        metrics["alpha_mask"] = dict(grid=mask_grid)
        for name, field in (("static", tr.st), ("dynamic", tr.dy)):
            field.updateAlphaMask(mask_grid)
            st = field.alphaMask_stats
            metrics["alpha_mask"][name] = dict(st, fraction=st["occupied"] / st["total"])
        metrics["train_masked"] = rodynrf.evaluate(tr, scene, frames="train", alpha_masks=True)
        if scene.heldout:
            metrics["heldout_masked"] = rodynrf.evaluate(tr, scene, frames="heldout", alpha_masks=True)
    if a.tracks > 0:
        H, W, frame = scene.H, scene.W, scene.T // 2
        query = track_queries(a.tracks, H, W).to(dev)
        focal = tr.focal()
        tracks, acc_d = rodynrf.render_tracks(tr.st, tr.dy, tr.pose_table().detach(), focal.detach() if torch.is_tensor(focal) else focal,
                                              frame, query, H, W, N_samples=tr.cfg["n_samples"], ray_type=tr.cfg["ray_type"])
        np.savez(os.path.join(a.out, "tracks.npz"), points=tracks.points.cpu().numpy(), pixels=tracks.pixels.cpu().numpy(),
                 disp=tracks.disp.cpu().numpy(), acc_d=acc_d.cpu().numpy(), query=query.cpu().numpy(), frame=frame,
                 frames_offset=tracks.frames_offset.cpu().numpy())
        metrics["tracks"] = dict(n=int(query.shape[0]), frame=frame)
    with open(os.path.join(a.out, "metrics.json"), "w") as f:
        json.dump(metrics, f, indent=1)
    print(json.dumps(summary(metrics)))


if __name__ == "__main__":
    main()
