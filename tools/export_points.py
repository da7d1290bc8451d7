#!/usr/bin/env python
"""Checkpoint pair -> the coloured point cloud one training camera sees (surface hits of its rays), on the device.

    python tools/export_points.py ckpt.th out.ply --frame K --size H W [--tau 0.5] [--dynamic-only | --static-only] [--world]
                                                  [--focal F] [--samples S] [--ray-type ndc|contract]

ckpt.th is the dynamic field's checkpoint and ckpt_static.th, next to it, the static field's (Trainer.save writes both);
the camera is frame K of the poses the checkpoint carries, the time that frame's, the focal length the checkpoint's unless
--focal gives one.  --tau: the opacity level of the hit (0.5: the median depth).  --dynamic-only / --static-only keep the
points whose hit sample belongs mostly to the dynamic / static field (owner >= / <= 0.5).  --world maps the points from field
coordinates to world space."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("ckpt")
    ap.add_argument("ply")
    ap.add_argument("--frame", type=int, required=True)
    ap.add_argument("--size", type=int, nargs=2, required=True, metavar=("H", "W"))
    ap.add_argument("--tau", type=float, default=0.5)
    only = ap.add_mutually_exclusive_group()
    only.add_argument("--dynamic-only", action="store_true")
    only.add_argument("--static-only", action="store_true")
    ap.add_argument("--world", action="store_true")
    ap.add_argument("--focal", type=float, default=None)
    ap.add_argument("--samples", type=int, default=-1)
    ap.add_argument("--ray-type", default="ndc", choices=("ndc", "contract"))
    a = ap.parse_args()
    import torch
    import rodynrf
    load_field = rodynrf.mesh.load_field
    ckpt = torch.load(a.ckpt, map_location="cpu", weights_only=False)
    poses = torch.as_tensor(ckpt["kwargs"]["se3_poses"], dtype=torch.float32)
    T = poses.shape[0]
    if not 0 <= a.frame < T:
        ap.error(f"--frame {a.frame} of a {T}-frame video")
    focal = a.focal if a.focal is not None else float(torch.as_tensor(ckpt["kwargs"]["focal_ratio_refine"]).reshape(-1)[0])
    root, ext = os.path.splitext(a.ckpt)
    dy, st = load_field(a.ckpt), load_field(root + "_static" + ext)
    H, W = a.size
    xyz, rgb, owner = rodynrf.point_cloud(st, dy, poses[a.frame, :3, :4], focal, H, W, 2.0 * a.frame / max(T - 1, 1) - 1.0,
                                          tau=a.tau, space="world" if a.world else "field",
                                          min_owner=0.5 if a.dynamic_only else None, max_owner=0.5 if a.static_only else None,
                                          N_samples=a.samples, ray_type=a.ray_type)
    rodynrf.write_ply(a.ply, xyz, None, colors=(rgb * 255.0).round().to(torch.uint8))
    print(f"{a.ply}: {xyz.shape[0]} points of {H * W} rays")


if __name__ == "__main__":
    main()
