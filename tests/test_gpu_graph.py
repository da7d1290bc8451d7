"""Trainer(graph=True): one training iteration (batch gather, every forward pass of train.py:1092-2311, both backward
phases) captured as a HIP graph and replayed.  A replay must be THE iteration the eager path computes on the same
parameters, ray indices, sampling jitter, white-background coins and iteration scalars -- all of which change from
replay to replay and reach the captured kernels through static device memory only (ABI 6: white_dev of
rdrf_composite_*, coef_dev of RdrfLossTerm)."""

import pytest
import torch

from _util import assert_close, pkg, record_margin

pytestmark = pytest.mark.gpu

# the coarse stages of the shipped configs (S = 13: the launch-bound shapes the graph exists for) at their full batch
# size, and a small Nvidia.txt shape
SHAPES = {
    "nvidia": dict(grid=[24, 26, 16], n_samples=24, batch_size=256, H=27, W=48, T=6),
    "nvidia_no_poses": {},
    "davis": {},
}


def _sync_eager_to(tr_e, tr_g):
    """the eager twin starts the iteration from the captured trainer's state: parameters, iteration, draws"""
    for se, sg in zip(tr_e.opt.state, tr_g.opt.state):
        se["p"].copy_(sg["p"])
    for f in tr_e.opt.fields:
        f._pack_epoch += 1   # packed weight images are stale
    if tr_g.optimize_poses:
        with torch.no_grad():
            tr_e.poses.copy_(tr_g.poses)
            tr_e.fov.copy_(tr_g.fov)
    tr_e.it = tr_g.it
    tr_e.rng.pool.copy_(tr_g.rng.pool)
    tr_e.rng.coins.copy_(tr_g.rng.coins)
    tr_e.rng.begin()   # frozen: only the cursors are reset


@pytest.mark.parametrize("name", ["nvidia", "nvidia_no_poses", "davis"])
def test_captured_iteration_replays_the_eager_iteration(name):
    S_ = pkg("step")
    dev = torch.device("cuda", 0)
    cfg = S_.scene_config(name, "stage0")
    cfg.update(SHAPES[name])
    if SHAPES[name]:
        cfg["focal"] = max(cfg["H"], cfg["W"]) / 2.0 * 3.0 ** 0.5
    tr_g = S_.Trainer(dict(cfg), dev, graph=True)
    tr_e = S_.Trainer(dict(cfg), dev)
    tr_e.rng = S_.GraphRng(dev)
    tr_e.rng.frozen = True
    tr_g.it = 30000   # every gate open, the ramped weights non-zero
    coins_seen = set()
    n_replays = 0
    for k in range(7):
        if k == 4:
            tr_g.it += 9000   # same gates (same graph), other iteration scalars: distortion ramp x 1.3, Temp_static x 0.81
        tr_g.step()
        replayed = bool(tr_g._graphs) and tr_g._graph_key() in tr_g._graphs
        n_replays += int(replayed)
        coins_seen.add(tuple(tr_g.rng.coins[:8].tolist()))
        _sync_eager_to(tr_e, tr_g)
        b = tr_e.data.make_batch(tr_e.it, cfg["batch_size"])
        tr_e._forward_backward(b, tv_between=True)
        for key in ("loss_dynamic", "loss_static"):
            assert_close(tr_g.last[key], tr_e.last[key], f"{key} at step {k}", rtol=2e-6)
        pairs = list(zip(tr_g.grad_flats, tr_e.grad_flats))
        if tr_g.optimize_poses:
            pairs += [(tr_g.poses.grad, tr_e.poses.grad), (tr_g.fov.grad, tr_e.fov.grad)]
        for j, (a, b_) in enumerate(pairs):
            assert float(b_.abs().max()) > 0
            rel = float((a - b_).norm() / b_.norm())
            # Two orders of the same fp32 atomic accumulation.  Measured with tools/graph/noise.py (profiles/r06_graph_noise.txt):
            # captured-vs-eager next to eager-vs-eager (two runs of ONE path) per buffer -- field buffers and pose table
            # <= 8.1e-6 / <= 8.1e-6; the field of view is ONE float that every ray's gradient is added to, with heavy
            # cancellation: 1.8e-4 captured-vs-eager, 6.1e-5 between two eager runs (davis, 8192 rays).  A captured launch
            # sequence takes the sorted scatter at every size (rdrf_scatter.hip scatter_mode), the eager twin the ray-tile
            # scatter below 300 k samples: the same distance as batched-vs-per-pass (tests/test_gpu_trainer.py: <= 8.9e-6,
            # bound 5e-5).  Bounds: 5e-5, and 2e-3 for that scalar.  A replay on stale inputs (a coin, a jitter vector, the
            # iteration scalars) moves every buffer by >= 1e-2.
            bound = 2e-3 if (tr_g.optimize_poses and j == len(pairs) - 1) else 5e-5
            record_margin(f"captured vs eager gradient (rel. L2 / {bound:g})", rel / bound)
            assert rel < bound, (k, j, rel)
        tr_g.finish_step()
    assert n_replays >= 5, n_replays            # iteration 0 of a key runs eagerly, the second captures, then replays
    assert len(tr_g._graphs) == 1                # the jump of the iteration counter did not re-capture
    assert len(coins_seen) >= 3, coins_seen      # the coins did change between the replays compared above
    if name == "nvidia":
        # upsample_volume_grid: new factor tensors and gradient buffers -- the captured iterations are dropped
        tr_g.upsample([30, 33, 20], 30)
        assert not tr_g._graphs
        for _ in range(3):
            loss = tr_g.step()
            tr_g.finish_step()
        assert len(tr_g._graphs) == 1 and torch.isfinite(loss)


def test_graph_training_run_reduces_loss():
    """the same short run as test_short_training_run_reduces_loss, through replays (Adam, TV and the learning-rate decay
    stay outside the graph and must keep acting on the buffers the captured kernels read)"""
    S_ = pkg("step")
    cfg = S_.balloon1_config("stage0")
    cfg.update(grid=[36, 40, 24], n_samples=48, batch_size=512, H=27, W=48, T=6)
    cfg["focal"] = max(cfg["H"], cfg["W"]) / 2.0 * 3.0 ** 0.5
    tr = S_.Trainer(cfg, torch.device("cuda", 0), graph=True)
    losses = []
    for _ in range(40):
        loss = tr.step()
        tr.finish_step()
        losses.append(float(loss.detach()))
    assert all(l == l and abs(l) < 1e6 for l in losses), losses
    assert len(tr._graphs) >= 1
    first, last = sum(losses[:5]) / 5, sum(losses[-5:]) / 5
    assert last < 0.9 * first, (first, last)


def test_graph_refuses_data_parallel_shards():
    S_ = pkg("step")
    cfg = S_.balloon1_config("stage0")
    cfg.update(grid=[24, 26, 16], n_samples=24, batch_size=64, H=27, W=48, T=6)
    tr = S_.Trainer(cfg, torch.device("cuda", 0), graph=True)
    with pytest.raises(RuntimeError, match="single-process"):
        tr.step(shard=(0, 2))
