"""Training on an array-backed scene (scene.Scene): the fused batch gather (rdrf_gather_batch) against torch indexing of
float tables built the way step.SyntheticScene builds its own, Scene as a drop-in for SyntheticScene, Trainer(data=scene)
in eager and captured form, the run driver Trainer.fit with the reference's resolution schedule, learning on an analytic
video, save / load of a run's state, evaluate()."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from _util import assert_close, pkg, record_margin

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the smallest shapes the kernels accept (tests/test_gpu_trainer.py SMALL)
SMALL = {
    "nvidia": dict(grid=[24, 26, 16], n_samples=24, batch_size=64),
    "nvidia_no_poses": dict(grid=[17, 19, 11], n_samples=13, batch_size=64),
}
T6, H27, W48 = 6, 27, 48


def _dev():
    return torch.device("cuda", 0)


def random_arrays(T, H, W, seed=0, poses=True):
    g = torch.Generator().manual_seed(seed)
    a = dict(rgb=(torch.rand(T, H, W, 3, generator=g) * 255).to(torch.uint8), flow_f=2.0 * torch.randn(T, H, W, 2, generator=g),
             flow_b=2.0 * torch.randn(T, H, W, 2, generator=g), flow_mask_f=torch.rand(T, H, W, generator=g) < 0.8,
             flow_mask_b=torch.rand(T, H, W, generator=g) < 0.8, disp=torch.rand(T, H, W, generator=g),
             fg_mask=torch.rand(T, H, W, generator=g) < 0.2)
    if poses:
        c2w = torch.eye(3, 4).repeat(T, 1, 1)
        c2w[:, 0, 3] = torch.linspace(-0.05, 0.05, T)
        a["poses"] = c2w
    return a


def small_cfg(name, **over):
    S_ = pkg("step")
    cfg = S_.scene_config(name, "stage0")
    cfg.update(SMALL[name])
    cfg.update(T=None, H=None, W=None)    # the scene's
    cfg.update(over)
    return cfg


@pytest.fixture(scope="module")
def scene_posed():
    SC = pkg("scene")
    a = random_arrays(T6, H27, W48)
    held = [(a["poses"][2], -0.2, a["rgb"][2])]
    return SC.Scene(**a, heldout=held, device=_dev())


@pytest.fixture(scope="module")
def scene_unposed():
    SC = pkg("scene")
    return SC.Scene(**random_arrays(T6, H27, W48, seed=1, poses=False), device=_dev())


# ---- the gather ----------------------------------------------------------------------------------------------------
def float_tables(a, T, H, W):
    """the per-pixel fp32 tables, built on the host as step.SyntheticScene builds its own (step.py: pix / col / row / view)"""
    total = T * H * W
    pix = torch.arange(total)
    col, row, view = pix % W, (pix // W) % H, pix // (W * H)
    rgb = a["rgb"].reshape(total, 3)
    t = dict(rgb=rgb.float() / 255 if rgb.dtype == torch.uint8 else rgb, flow_f=a["flow_f"].reshape(total, 2),
             flow_b=a["flow_b"].reshape(total, 2), grid=torch.stack([col.float() + 0.5, row.float() + 0.5], -1),
             px=torch.stack([col.float(), row.float()], -1), view=view, ts=view.float() * (2.0 / (T - 1)) - 1.0,
             disp=a["disp"].reshape(total) if a.get("disp") is not None else torch.zeros(total),
             fg=a["fg_mask"].reshape(total).float() if a.get("fg_mask") is not None else torch.zeros(total),
             mask_f=a["flow_mask_f"].reshape(total, 1).float(), mask_b=a["flow_mask_b"].reshape(total, 1).float())
    return {k: v.to(_dev()) for k, v in t.items()}


def gather_ids(N, total, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, total, (N,), generator=g)
    if N >= 1:
        ids[-1] = total - 1                 # the last pixel: its colour word would end past the uint8 table
    if N >= 4:
        ids[0] = 0
        ids[2] = ids[1]                     # duplicates
        ids[3] = total - 1
    return ids


@pytest.mark.parametrize("rgb_dtype", ["uint8", "float32"])
@pytest.mark.parametrize("optional", [True, False])
def test_gather_matches_indexing_of_float_tables(rgb_dtype, optional):
    SC = pkg("scene")
    T, H, W = 3, 5, 7
    total = T * H * W
    a = random_arrays(T, H, W, seed=3, poses=False)
    a["rgb"] = (torch.arange(total * 3) % 256).to(torch.uint8)[torch.randperm(total * 3, generator=torch.Generator().manual_seed(1))
                                                               ].view(T, H, W, 3)     # every byte value
    assert a["rgb"].unique().numel() == 256
    if not optional:
        a["disp"], a["fg_mask"] = None, None
    ref = float_tables(a, T, H, W)
    if rgb_dtype == "float32":
        a = dict(a, rgb=a["rgb"].float() / 255)
    sc = SC.Scene(**a, device=_dev())
    assert sc.rgb.dtype == getattr(torch, rgb_dtype)
    for N in (0, 1, 63, 64, 65, 257):
        ids, ids2 = gather_ids(N, total, N).to(_dev()), gather_ids(N, total, 1000 + N).flip(0).to(_dev())
        b = sc.make_batch(0, N, ids=(ids, ids2), check=True)
        assert set(b) == {"ids", "ts", "ts_rand", "grid", "px", "view", "rgb", "disp", "fg", "flow_f", "flow_b", "mask_f", "mask_b"}
        assert torch.equal(b["ids"], ids)
        for k in ("ts", "grid", "px", "view", "rgb", "disp", "fg", "flow_f", "flow_b", "mask_f", "mask_b"):
            want = ref[k][ids]
            assert b[k].dtype == want.dtype and b[k].shape == want.shape, (N, k, b[k].dtype, b[k].shape)
            assert torch.equal(b[k], want), (N, k)
        assert torch.equal(b["ts_rand"], ref["ts"][ids2]) and torch.equal(b["ts_rand"], sc.ts_of(ids2)), N
        if N >= 4:
            assert ids[0] == 0 and ids[1] == ids[2] and ids[-1] == total - 1
    if not optional:
        assert float(b["disp"].abs().max()) == 0.0 and float(b["fg"].abs().max()) == 0.0
    with pytest.raises(L_().RdrfError):
        sc.make_batch(0, 2, ids=(torch.tensor([0, total], device=_dev()), torch.tensor([0, 1], device=_dev())), check=True)


def L_():
    return pkg()


def test_gather_of_an_empty_batch_touches_nothing(scene_posed):
    L = L_()
    sc = scene_posed
    bufs = {n: torch.full((8,), 7.0 if n != "view" else 7, dtype=torch.int64 if n == "view" else torch.float32, device=_dev())
            for n in L.BATCH_OUTPUTS}
    out = L.BatchC(*(C.c_void_p(bufs[n].data_ptr()) for n in L.BATCH_OUTPUTS))
    ids = torch.zeros(4, dtype=torch.int64, device=_dev())
    rc = L.lib.rdrf_gather_batch(C.byref(sc._tables), L.ptr(ids), L.ptr(ids), 0, C.byref(out), L.stream_of(ids))
    torch.cuda.synchronize()
    assert rc == 0 and all(bool((b == 7).all()) for b in bufs.values())
    # ... and a NULL output is refused, not dereferenced
    out.px = None
    assert L.lib.rdrf_gather_batch(C.byref(sc._tables), L.ptr(ids), L.ptr(ids), 4, C.byref(out), L.stream_of(ids)) < 0
    assert b"RdrfBatch" in L.lib.rdrf_last_error()
    b = sc.make_batch(0, 0, ids=(ids[:0], ids[:0]))
    assert b["rgb"].shape == (0, 3) and b["mask_f"].shape == (0, 1) and b["view"].dtype == torch.int64


def test_scene_is_a_drop_in_for_the_synthetic_scene():
    """a Scene built from a SyntheticScene's own tensors returns the same make_batch dict, bit for bit"""
    S_, SC = pkg("step"), pkg("scene")
    T, H, W = 4, 12, 16
    cfg = dict(T=T, H=H, W=W, focal=W / 2.0 * math.sqrt(3.0))
    syn = S_.SyntheticScene(cfg, _dev())
    sc = SC.Scene(syn.rgb.view(T, H, W, 3), syn.flow_f.view(T, H, W, 2), syn.flow_b.view(T, H, W, 2), syn.flow_mask_f.view(T, H, W),
                  syn.flow_mask_b.view(T, H, W), disp=syn.disp.view(T, H, W), fg_mask=syn.fgmask.view(T, H, W), focal=cfg["focal"],
                  device=_dev())
    assert sc.total == syn.total and torch.equal(sc.focal, syn.focal) and sc.focal.dtype == syn.focal.dtype
    bs = 96
    for it, shard in ((0, None), (5, None), (5, (1, 2)), (7, (0, 3))):
        ids = (syn.batch(it, bs, 0), syn.batch(it, bs, 1))
        want, got = syn.make_batch(it, bs, shard=shard, ids=ids), sc.make_batch(it, bs, shard=shard, ids=ids)
        assert list(got) == list(want)
        for k in want:
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
            assert torch.equal(got[k], want[k]), (it, shard, k)
        assert got["ids"].shape[0] == (bs if shard is None else bs // shard[1])
    assert torch.equal(sc.ts_of(ids[0]), syn.ts_of(ids[0]))


# ---- the trainer on a scene ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nvidia", "nvidia_no_poses"])
def test_trainer_on_a_scene_eager_and_captured(name, scene_posed, scene_unposed):
    """one eager step and captured iterations of Trainer(data=scene); a replay is the eager iteration on the same state, by
    the criterion of tests/test_gpu_graph.py (losses at 2e-6, gradients at 5e-5 relative L2, the field of view -- one float
    every ray adds to -- at 2e-3)."""
    S_ = pkg("step")
    scene = scene_posed if name == "nvidia" else scene_unposed
    cfg = small_cfg(name)
    tr_g = S_.Trainer(dict(cfg), _dev(), graph=True, data=scene)
    tr_e = S_.Trainer(dict(cfg), _dev(), data=scene)
    assert tr_e.data is scene and (tr_e.cfg["T"], tr_e.cfg["H"], tr_e.cfg["W"]) == (T6, H27, W48)
    assert torch.equal(tr_e.pose_table().detach(), scene.poses)
    if not tr_e.optimize_poses:
        assert tr_e.focal() is scene.focal
    loss = tr_e.step()           # the plain eager path, its own draws
    tr_e.finish_step()
    assert torch.isfinite(loss)
    tr_e.rng = S_.GraphRng(_dev())
    tr_e.rng.frozen = True
    tr_g.it = 30000              # every gate open, the ramped weights non-zero
    n_replays = 0
    for k in range(3):
        loss_g = tr_g.step()
        replayed = bool(tr_g._graphs) and tr_g._graph_key() in tr_g._graphs
        n_replays += int(replayed)
        assert torch.isfinite(loss_g)
        # the eager twin starts the iteration from the captured trainer's state: parameters, iteration, draws
        for se, sg in zip(tr_e.opt.state, tr_g.opt.state):
            se["p"].copy_(sg["p"])
        for f in tr_e.opt.fields:
            f._pack_epoch += 1
        if tr_g.optimize_poses:
            with torch.no_grad():
                tr_e.poses.copy_(tr_g.poses)
                tr_e.fov.copy_(tr_g.fov)
        tr_e.it = tr_g.it
        tr_e.rng.pool.copy_(tr_g.rng.pool)
        tr_e.rng.coins.copy_(tr_g.rng.coins)
        tr_e.rng.begin()
        tr_e._forward_backward(scene.make_batch(tr_e.it, cfg["batch_size"]), tv_between=True)
        for key in ("loss_dynamic", "loss_static"):
            assert_close(tr_g.last[key], tr_e.last[key], f"{key} at step {k}", rtol=2e-6)
        pairs = list(zip(tr_g.grad_flats, tr_e.grad_flats))
        if tr_g.optimize_poses:
            pairs += [(tr_g.poses.grad, tr_e.poses.grad), (tr_g.fov.grad, tr_e.fov.grad)]
        for j, (x, y) in enumerate(pairs):
            assert float(y.abs().max()) > 0
            rel = float((x - y).norm() / y.norm())
            bound = 2e-3 if (tr_g.optimize_poses and j == len(pairs) - 1) else 5e-5
            record_margin(f"captured vs eager gradient on a scene (rel. L2 / {bound:g})", rel / bound)
            assert rel < bound, (k, j, rel)
        tr_g.finish_step()
    assert n_replays >= 1 and len(tr_g._graphs) == 1


def test_trainer_refuses_a_config_of_another_shape(scene_posed, scene_unposed):
    S_ = pkg("step")
    with pytest.raises(ValueError, match="H"):
        S_.Trainer(small_cfg("nvidia", H=H27 + 1), _dev(), data=scene_posed)
    with pytest.raises(ValueError, match="poses"):
        S_.Trainer(small_cfg("nvidia"), _dev(), data=scene_unposed)   # optimize_poses=False and nothing to hold them at


def test_trainer_step_on_a_shard_of_a_scene(scene_posed):
    S_ = pkg("step")
    tr = S_.Trainer(small_cfg("nvidia"), _dev(), data=scene_posed)
    loss = tr.step(shard=(1, 2))
    tr.finish_step()
    assert torch.isfinite(loss) and tr.it == 1


# ---- fit: the resolution schedule ----------------------------------------------------------------------------------
def test_fit_follows_the_resolution_schedule(scene_unposed):
    S_ = pkg("step")
    cfg = small_cfg("nvidia_no_poses", upsamp_list=[3, 6, 9, 12], n_iters=16, N_voxel_init=16 ** 3, N_voxel_final=32 ** 3,
                    batch_size=256)
    del cfg["grid"], cfg["n_samples"]          # the trainer starts at the schedule's first stage
    stages = S_.resolution_stages(cfg)
    assert [s[0] for s in stages] == [0, 4, 7, 10, 13] and stages[0][1:] == ([17, 19, 11], 13)
    assert all(a[1] != b[1] and a[2] < b[2] for a, b in zip(stages, stages[1:]))
    tr = S_.Trainer(cfg, _dev(), data=scene_unposed)
    assert (tr.cfg["grid"], tr.cfg["n_samples"]) == stages[0][1:]
    assert tr.opt_focal.param_groups[0]["lr"] == 0.0 and tr.opt_pose.param_groups[0]["lr"] == tr.lr_pose
    seen, losses = [], []

    def callback(trainer, it, loss):
        assert trainer is tr and trainer.it == it + 1
        seen.append(it)
        losses.append(loss)
        k = sum(1 for u in cfg["upsamp_list"] if u <= it)      # the stage iteration it + 1 runs on
        grid, n_samples = stages[k][1:]
        assert trainer.cfg["grid"] == grid and trainer.cfg["n_samples"] == n_samples
        for f in (trainer.st, trainer.dy):
            assert f.gridSize.tolist() == grid
            assert list(f.density_plane[0].shape[-2:]) == [grid[1], grid[0]]
        if it in cfg["upsamp_list"]:       # right after an upsample: a new Adam, restarted rates (train.py:2589-2606)
            assert trainer.opt.t == 0 and trainer.opt.lr0 == 0.02 and trainer.opt.lr1 == 1e-3
            assert all(float(s["m"].abs().max()) == 0.0 and float(s["v"].abs().max()) == 0.0 for s in trainer.opt.state)
            assert all(s["p"].numel() == f.flatten_params_().numel() for s, f in zip(trainer.opt.state, trainer.opt.fields))
            assert trainer.opt_pose.param_groups[0]["lr"] == trainer.lr_pose
            assert trainer.opt_focal.param_groups[0]["lr"] == (trainer.lr_pose if it >= cfg["upsamp_list"][3] else 0.0)
        elif it > 0 and it - 1 not in cfg["upsamp_list"]:
            assert trainer.opt.t > 1 and trainer.opt.lr0 < 0.02

    last = tr.fit(callback=callback)
    assert tr.it == 16 and seen == list(range(16)) and last is losses[-1]
    assert bool(torch.isfinite(torch.stack(losses)).all())
    assert tr.fit(n_iters=5) is None and tr.it == 16           # stops at cfg["n_iters"]
    tr2 = S_.Trainer(dict(cfg, grid=stages[0][1], n_samples=stages[0][2]), _dev(), data=scene_unposed)
    tr2.fit(n_iters=2)
    assert tr2.it == 2 and tr2.cfg["grid"] == stages[0][1]
    tr2.fit(n_iters=2)                                             # iteration 3 is in the list
    assert tr2.it == 4 and tr2.cfg["grid"] == stages[1][1]


# ---- learning ------------------------------------------------------------------------------------------------------
def analytic_video(T=4, H=24, W=32):
    """a disc translating over a fixed textured plane, seen by a fixed camera: exact flows, masks, disparity, poses"""
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    plane = torch.stack([0.5 + 0.3 * torch.sin(0.7 * x) * torch.cos(0.5 * y), 0.5 + 0.3 * torch.cos(0.4 * x + 0.3 * y),
                         0.4 + 0.2 * torch.sin(0.9 * y)], -1)
    step, radius = 4.0, 5.0
    disc = lambda t: (x - (8.0 + step * t)) ** 2 + (y - 12.0) ** 2 <= radius ** 2
    rgb, ff, fb, mf, mb, disp, fg = [], [], [], [], [], [], []
    for t in range(T):
        d = disc(t)
        rgb.append(torch.where(d[..., None], torch.tensor([0.9, 0.2, 0.1]), plane))
        fg.append(d)
        disp.append(torch.where(d, torch.tensor(0.8), torch.tensor(0.2)))
        z = torch.zeros(H, W, 2)
        f, b = z.clone(), z.clone()
        f[..., 0][d] = step
        b[..., 0][d] = -step
        ff.append(f)
        fb.append(b)
        # a correspondence exists where a neighbour frame exists and the pixel is not covered by the disc there
        mf.append((d | ~disc(t + 1)) if t + 1 < T else torch.zeros(H, W, dtype=torch.bool))
        mb.append((d | ~disc(t - 1)) if t >= 1 else torch.zeros(H, W, dtype=torch.bool))
    st = torch.stack
    return dict(rgb=st(rgb), flow_f=st(ff), flow_b=st(fb), flow_mask_f=st(mf), flow_mask_b=st(mb), disp=st(disp), fg_mask=st(fg),
                poses=torch.eye(3, 4).repeat(T, 1, 1))


def test_fit_learns_an_analytic_video(capsys):
    """200 iterations at a fixed seed on the analytic video: the photometric term (3 x the mean squared error of the composited
    colours against the video's, train.py:1323) averaged over the last 20 iterations is lower than over the first 20.
    Measured: profiles/r11_scene_fit.txt."""
    S_, SC = pkg("step"), pkg("scene")
    scene = SC.Scene(**analytic_video(), device=_dev(), seed=11)
    cfg = small_cfg("nvidia", batch_size=256)
    torch.manual_seed(0)
    tr = S_.Trainer(cfg, _dev(), data=scene)
    photo = []
    tr.fit(n_iters=200, callback=lambda trainer, it, loss: photo.append(trainer.terms[0].values[0].clone()))
    photo = torch.stack(photo).cpu()
    first, last = float(photo[:20].mean()), float(photo[-20:].mean())
    with capsys.disabled():
        print(f"\nscene fit, analytic video T=4 24x32, 200 iterations of 256 rays, grid {cfg['grid']}, {cfg['n_samples']} samples: "
              f"photometric term first 20 = {first:.6f}, last 20 = {last:.6f}")
    assert bool(torch.isfinite(photo).all()) and tr.it == 200
    assert last < first, (first, last)


# ---- state of a run ------------------------------------------------------------------------------------------------
def _draws(rng, S, n=140):
    """the next draws of a StepRng: n jitter vectors (enough to refill the device pool once) and coins"""
    out = []
    for _ in range(n):
        out.append(rng.jitter(S, "ndc", _dev())[0].clone())
        out.append(torch.tensor(float(rng.coin())))
    return out


def test_save_and_load_restore_a_run(tmp_path, scene_unposed):
    S_, SC = pkg("step"), pkg("scene")
    import rodynrf
    scene = scene_unposed
    cfg = small_cfg("nvidia_no_poses", n_iters=1000)    # a visible decay of every rate per step
    a = S_.Trainer(dict(cfg), _dev(), data=scene)
    a.fit(n_iters=5)
    prefix = str(tmp_path / "run")
    a.save(prefix)
    assert sorted(os.listdir(tmp_path)) == ["run.th", "run_state.th", "run_static.th"]
    draws_a = _draws(a.rng, cfg["n_samples"])          # (moves a's draws on: a is not stepped again)
    # a second scene object with ANOTHER sampler seed: load() restores the saved one
    other = SC.Scene(**random_arrays(T6, H27, W48, seed=1, poses=False), device=_dev(), seed=99)
    assert not torch.equal(other.batch(5, 64, 0), scene.batch(5, 64, 0))
    b = S_.Trainer(dict(cfg), _dev(), data=other)
    b.load(prefix)
    assert b.it == a.it == 5 and b.cfg["grid"] == a.cfg["grid"] and b.cfg["n_samples"] == a.cfg["n_samples"]
    for sa, sb in zip(a.opt.state, b.opt.state):
        for k in ("p", "m", "v"):
            assert torch.equal(sa[k], sb[k]), k
        assert float(sa["m"].abs().max()) > 0
    for fa, fb in ((a.st, b.st), (a.dy, b.dy)):
        for (ka, va), (kb, vb) in zip(fa.state_dict().items(), fb.state_dict().items()):
            assert ka == kb and torch.equal(va, vb) and va.stride() == vb.stride(), ka
    assert (a.opt.t, a.opt.lr0, a.opt.lr1) == (b.opt.t, b.opt.lr0, b.opt.lr1) and a.opt.lr0 < 0.02
    assert torch.equal(a.poses, b.poses) and torch.equal(a.fov, b.fov) and not torch.equal(a.poses.detach(), scene.poses)
    for oa, ob in ((a.opt_pose, b.opt_pose), (a.opt_focal, b.opt_focal)):
        assert oa.param_groups[0]["lr"] == ob.param_groups[0]["lr"]
        (sa,), (sb,) = oa.state.values(), ob.state.values()
        assert float(sa["step"]) == float(sb["step"]) == 5
        assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"])
    assert a.opt_pose.param_groups[0]["lr"] < a.lr_pose
    for it in (5, 6):
        for which in (0, 1):
            assert torch.equal(a.data.batch(it, 64, which), b.data.batch(it, 64, which))
    draws_b = _draws(b.rng, cfg["n_samples"])
    assert len(draws_a) == len(draws_b) and all(torch.equal(x.cpu(), y.cpu()) for x, y in zip(draws_a, draws_b))
    # the reference-format pair: the reload recipe of train.py:433-447, then the same render bits as the live fields
    fields = []
    for path, cls in ((prefix + "_static.th", rodynrf.TensorVMSplit), (prefix + ".th", rodynrf.TensorVMSplit_TimeEmbedding)):
        ckpt = torch.load(path, map_location="cpu", weights_only=False)
        kwargs = dict(ckpt["kwargs"])
        poses_mtx, focal = kwargs.pop("se3_poses"), kwargs.pop("focal_ratio_refine")
        assert poses_mtx.shape == (T6, 3, 4) and torch.equal(poses_mtx, rodynrf.pose_to_mtx(a.poses.detach()).cpu())
        assert torch.equal(focal, a.focal().detach().cpu())
        kwargs.update({"device": _dev()})
        m = cls(**kwargs)
        m.load(ckpt)
        fields.append(m)
    want = rodynrf.render_frame(a.st, a.dy, a.poses.detach(), a.focal().detach(), 1, H27, W48, N_samples=13)
    got = rodynrf.render_frame(fields[0], fields[1], a.poses.detach(), a.focal().detach(), 1, H27, W48, N_samples=13)
    assert torch.equal(want[0], got[0]) and torch.equal(want[1], got[1]) and bool(torch.isfinite(want[0]).all())
    # a run that was saved after an upsample loads into a trainer built at the first stage
    a.upsample([20, 22, 13], 16)
    a.save(prefix)
    c = S_.Trainer(dict(cfg), _dev(), data=scene)
    c.load(prefix)
    assert c.cfg["grid"] == [20, 22, 13] and c.cfg["n_samples"] == 16 and c.st.gridSize.tolist() == [20, 22, 13]
    assert all(torch.equal(sa["p"], sc["p"]) for sa, sc in zip(a.opt.state, c.opt.state))
    loss = c.step()
    c.finish_step()
    assert torch.isfinite(loss)


def test_resumed_run_is_bit_identical_in_the_deterministic_build(tmp_path):
    """tools/resume_check.py under librodynrf_det.so (selected as tests/test_gpu_deterministic.py selects it): 5 iterations,
    save, load into a new trainer; 3 further iterations equal the uninterrupted run's in every parameter and moment bit"""
    env = dict(os.environ, RDRF_DETERMINISTIC="1")
    env.pop("RDRF_LIB", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "resume_check.py"), str(tmp_path)], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "deterministic=1 it=8/8 elements that differ: 0 " in r.stdout, r.stdout


# ---- evaluate ------------------------------------------------------------------------------------------------------
def test_evaluate_equals_the_public_calls_made_by_hand(scene_posed):
    S_, SC = pkg("step"), pkg("scene")
    import rodynrf
    scene = scene_posed
    tr = S_.Trainer(small_cfg("nvidia"), _dev(), data=scene)
    S = tr.cfg["n_samples"]
    ev = SC.evaluate(tr, scene, frames="train")
    assert len(ev["psnr"]) == len(ev["ssim"]) == T6
    rgb, _ = rodynrf.render_frame(tr.st, tr.dy, tr.pose_table(), tr.focal(), 4, H27, W48, N_samples=S, ray_type="ndc")
    ref = scene.rgb[4 * H27 * W48: 5 * H27 * W48].view(H27, W48, 3).float() / 255
    assert ev["psnr"][4] == float(rodynrf.psnr(rgb, ref).double()) and ev["ssim"][4] == float(rodynrf.ssim(rgb, ref))
    assert ev["psnr_mean"] == pytest.approx(sum(ev["psnr"]) / T6) and ev["ssim_mean"] == pytest.approx(sum(ev["ssim"]) / T6)
    assert all(math.isfinite(v) for v in ev["psnr"] + ev["ssim"])
    ev = SC.evaluate(tr, scene)           # the held-out view
    c2w, t, img = scene.heldout[0]
    rgb, _ = rodynrf.render_view(tr.st, tr.dy, c2w, tr.focal(), H27, W48, t, N_samples=S, ray_type="ndc", maps=False)
    assert ev["psnr"] == [float(rodynrf.psnr(rgb, img).double())] and ev["ssim"] == [float(rodynrf.ssim(rgb, img))]
    with pytest.raises(ValueError):
        SC.evaluate(tr, scene, frames="test")
