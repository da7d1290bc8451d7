"""One training step of a small (or the benchmark) scene; saves the loss, the two flat gradient buffers and, where the
trainer optimises them, the gradients of the pose table and the field of view.  Run with
RDRF_DETERMINISTIC=1 for the fixed-point build:   python tools/det_check.py out.pt [small|bench] [config]"""
import importlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
S_ = importlib.import_module("robust-dynrf_amd.step")
out, size = sys.argv[1], (sys.argv[2] if len(sys.argv) > 2 else "small")
name = sys.argv[3] if len(sys.argv) > 3 else "nvidia"
cfg = S_.scene_config(name, "stage0")
if size == "small":
    cfg.update(grid=[24, 26, 16], n_samples=40, batch_size=256, H=27, W=48, T=6)
    cfg["focal"] = max(cfg["H"], cfg["W"]) / 2.0 * 3.0 ** 0.5
torch.manual_seed(0)
tr = S_.Trainer(cfg, torch.device("cuda", 0))
tr.it = 9000
loss = tr.step()
torch.cuda.synchronize()
got = {"loss": loss.cpu(), "flats": [f.detach().cpu() for f in tr.grad_flats]}
if tr.optimize_poses:
    got.update(poses_grad=tr.poses.grad.cpu(), fov_grad=tr.fov.grad.cpu())
torch.save(got, out)
