"""Resume of a run from Trainer.save / Trainer.load:   python tools/resume_check.py DIR [config]
k = 5 iterations, save, 3 more (the uninterrupted run); a new trainer on the same scene loads the state and runs the same
3.  Prints the number of parameter / moment elements that differ.  Under RDRF_DETERMINISTIC=1 (librodynrf_det.so: gradients
independent of the order of their accumulation) every bit must agree and the exit status says so; the product build's
atomics leave fp32 accumulation noise between ANY two runs, so there the differences are reported only."""
import importlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
S_ = importlib.import_module("robust-dynrf_amd.step")
L = importlib.import_module("robust-dynrf_amd._lib")
Scene = importlib.import_module("robust-dynrf_amd.scene").Scene


def random_scene(T, H, W, device, seed=0, poses=True):
    g = torch.Generator().manual_seed(seed)
    c2w = torch.eye(3, 4).repeat(T, 1, 1)
    c2w[:, 0, 3] = torch.linspace(-0.05, 0.05, T)
    return Scene((torch.rand(T, H, W, 3, generator=g) * 255).to(torch.uint8), 2.0 * torch.randn(T, H, W, 2, generator=g),
                 2.0 * torch.randn(T, H, W, 2, generator=g), torch.rand(T, H, W, generator=g) < 0.8,
                 torch.rand(T, H, W, generator=g) < 0.8, disp=torch.rand(T, H, W, generator=g),
                 fg_mask=torch.rand(T, H, W, generator=g) < 0.2, poses=c2w if poses else None, device=device)


def main():
    out, name = sys.argv[1], (sys.argv[2] if len(sys.argv) > 2 else "nvidia_no_poses")
    dev = torch.device("cuda", 0)
    cfg = S_.scene_config(name, "stage0")
    cfg.update(grid=[17, 19, 11], n_samples=13, batch_size=64, H=None, W=None, T=None)
    scene = random_scene(6, 27, 48, dev, poses=not cfg["optimize_poses"])
    a = S_.Trainer(dict(cfg), dev, data=scene)
    a.fit(n_iters=5)
    prefix = os.path.join(out, "run")
    a.save(prefix)
    a.fit(n_iters=3)
    b = S_.Trainer(dict(cfg), dev, data=scene)
    b.load(prefix)
    b.fit(n_iters=3)
    pairs = [(sa[k], sb[k]) for sa, sb in zip(a.opt.state, b.opt.state) for k in ("p", "m", "v")]
    if a.optimize_poses:
        pairs += [(a.poses, b.poses), (a.fov, b.fov)]
    differ = sum(int((x != y).sum()) for x, y in pairs)
    worst = max(float((x - y).abs().max() / x.abs().max().clamp_min(1e-30)) for x, y in pairs)
    print(f"resume: deterministic={int(L.DETERMINISTIC)} it={a.it}/{b.it} elements that differ: {differ} "
          f"(worst max-norm distance {worst:.2e})")
    ok = a.it == b.it == 8 and (differ == 0 or not L.DETERMINISTIC)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
