"""Host logic of robust-dynrf_amd/step.py that needs no GPU: the pass-batching plan and the draw order of the pooled
jitter generator (the batched and the per-pass paths must consume the same random numbers in the same order)."""
import collections
import types

import pytest
import torch

from _util import pkg


def test_batch_groups_respect_the_sample_cap(monkeypatch):
    S_ = pkg("step")
    monkeypatch.setattr(S_, "BATCH_MAX_SAMPLES", 6_000_000)
    assert S_.batch_groups(range(4), 4096 * 115) == [[0, 1, 2, 3]]                 # benchmark shape: one call
    assert S_.batch_groups([1, 2, 3], 4096 * 270) == [[1, 2, 3]]                   # final stage
    assert S_.batch_groups([1, 2, 3], 4096 * 578) == [[1, 2], [3]]                 # 640^3 grid: two passes at a time
    assert S_.batch_groups(range(4), 4096 * 578) == [[0, 1], [2, 3]]
    assert S_.batch_groups(range(4), 8192 * 221) == [[0, 1, 2], [3]]               # DAVIS final
    assert S_.batch_groups([2, 3], 10 ** 9) == [[2], [3]]                          # a pass larger than the cap: alone
    for idxs, n in (([0, 1, 2, 3], 1), ([1, 2, 3], 5_000_000), ([5], 7)):
        g = S_.batch_groups(idxs, n)
        assert [k for grp in g for k in grp] == list(idxs) and all(len(grp) * n <= max(n, 6_000_000) for grp in g)


def test_step_rng_pool_and_coin_streams():
    """StepRng: the coins come from its own seeded generator (the same sequence whatever happens in between); the
    jitter vectors are consecutive 64-float-aligned slices of one pooled uniform draw, so taking (jitter, coin) for four
    passes up front (ray_passes) or one pass at a time (ray_pass) consumes the same values in the same order."""
    S_ = pkg("step")
    dev = torch.device("cpu")
    a, b = S_.StepRng(seed=11), S_.StepRng(seed=11)
    coins_a = [a.coin() for _ in range(16)]
    coins_b = []
    for _ in range(16):
        b.jitter(115, "ndc", dev)
        torch.rand(7)                                   # unrelated work on the global generator in between
        coins_b.append(b.coin())
    assert coins_a == coins_b and 0 < sum(coins_a) < 16
    c = S_.StepRng(seed=3)
    j0 = c.jitter(115, "ndc", dev)[0]
    pool = c._pool
    c.coin()
    j1 = c.jitter(115, "ndc", dev)[0]
    assert j0.shape == (115,) and torch.equal(j0, pool[0:115]) and torch.equal(j1, pool[128:243])
    jo = c.jitter(221, "contract", dev)
    assert jo[0].shape[0] == 221 - 221 // 2 + 1 and jo[1].shape[0] == 221 // 2 + 1
    assert torch.equal(jo[0], pool[256:256 + 111 + 1]) and torch.equal(jo[1], pool[384:384 + 111])
    assert float(pool.min()) >= 0.0 and float(pool.max()) < 1.0


N_RAYS, N_SAMPLES = 4, 3
PASS_NAMES = ("A", "B", "C", "D", "E", "P1", "P2", "P3", "P4")


class _StubIteration:
    """A Trainer whose fields, sampler, compositor and loss kernels are CPU stubs that log what step.run_passes does with
    them: ("jitter",) / ("coin",) per draw, ("sample", pass, box) per sampleXYZ, ("st" | "dy", passes, rgb flag, grad
    mode) per field call, ("composite", pass, had a dynamic call) per raw2outputs.  sampleXYZ numbers the passes in call
    order through the z values it returns; a field call reads the passes it covers back from them."""

    def __init__(self, S_, monkeypatch, name, batched, dead_work, it):
        self.S_, self.log, self.n_sampled = S_, [], 0
        N, S = N_RAYS, N_SAMPLES
        cfg = S_.scene_config(name, "stage0")
        cfg.update(n_samples=S, batch_size=N)
        tr = object.__new__(S_.Trainer)
        tr.cfg, tr.it, tr.batch_passes, tr.dead_work, tr.dp_exact_stats = cfg, it, batched, dead_work, False
        tr.optimize_poses, tr._dyn, tr._c2w_fixed = cfg["optimize_poses"], None, None
        tr.opt = types.SimpleNamespace(ex=types.SimpleNamespace(active=False))
        tr.data = types.SimpleNamespace(poses=torch.zeros(cfg["T"], 9), focal=torch.tensor(100.0))
        tr.poses, tr.fov = torch.nn.Parameter(torch.zeros(cfg["T"], 9)), torch.nn.Parameter(torch.full((1,), 0.5))
        tr.st, tr.dy, tr.rng = self._field("st"), self._field("dy"), self
        self.tr = tr
        terms = types.SimpleNamespace(total=lambda: torch.zeros(()))
        terms.add = lambda *a, **k: terms
        tr._loss_terms = lambda: terms
        # rays that require grad exactly where the real ones do: when they come from a live pose table / focal
        rays_of = lambda ids, poses, focal, *a, **k: torch.zeros(ids.shape[0], 6) + 0.0 * poses.sum() + 0.0 * torch.as_tensor(focal).sum()
        for fn, stub in (("sampleXYZ", self._sample), ("raw2outputs", self._composite), ("generate_rays", rays_of),
                         ("pose_to_mtx", lambda p: torch.zeros(p.shape[0], 3, 4)), ("gather_rows", lambda t, i: t[i]),
                         ("induce_flow", lambda *a, **k: (torch.zeros(N, 2), torch.zeros(N))),
                         ("distloss_rays", lambda *a: torch.zeros(())), ("frame_depth_loss", lambda *a, **k: torch.zeros(()))):
            monkeypatch.setattr(S_, fn, stub)

    def batch(self):
        N = N_RAYS
        z1, z2 = torch.zeros(N), torch.zeros(N, 2)
        return dict(ids=torch.arange(N), ts=z1, ts_rand=z1, rgb=torch.zeros(N, 3), disp=z1, fg=z1, grid=z2, px=z2,
                    view=torch.zeros(N, dtype=torch.long), flow_f=z2, flow_b=z2, mask_f=z1[:, None], mask_b=z1[:, None])

    # the rng
    def jitter(self, S, ray_type, device):
        self.log.append(("jitter",))
        return torch.zeros(S), None

    def coin(self):
        self.log.append(("coin",))
        return False

    def _sample(self, field, rays, S, ray_type="ndc", is_train=False, jitter=None, jitter_outer=None):
        assert (jitter is not None) == is_train
        k, self.n_sampled = self.n_sampled, self.n_sampled + 1
        self.log.append(("sample", k, field.name))
        N = rays.shape[0]
        return torch.zeros(N, S, 3), torch.full((N, S), float(k)), torch.ones(N, S, dtype=torch.bool)

    def _field(self, name):
        it, dyn = self, name == "dy"

        class StubField:
            def __call__(self, rays, ts, te, xyz, z, valid, is_train=False, ray_type="ndc", rgb=True):
                assert rays.shape[0] == ts.shape[0] == xyz.shape[0] == z.shape[0] == valid.shape[0]
                it.log.append((name, [int(v) for v in z[::N_RAYS, 0]], rgb, torch.is_grad_enabled()))
                w = torch.ones_like(z)
                return it.S_.FieldOut(None, None, w if dyn else None, xyz, w, xyz if dyn else None,
                                      None if rgb is False else xyz + 1.0, w, z, w)

            def get_forward_backward_scene_flow(self, pts, ts):
                return torch.zeros_like(pts), torch.zeros_like(pts)

        f = StubField()
        f.name = name
        return f

    def _composite(self, rgb_s, sigma_s, rgb_d, sigma_d, dists, blending, z_vals, rays, is_train=False, ray_type="ndc",
                   add_white_bg=None):
        assert rgb_s.shape == rgb_d.shape == (*sigma_s.shape, 3) and sigma_d.shape == blending.shape == dists.shape == sigma_s.shape
        dynamic = bool(sigma_d.any())   # the stub fields return ones: zeros stand in for an absent dynamic field
        assert dynamic == bool(blending.any()) and (dynamic or not bool(rgb_d.any()))
        self.log.append(("composite", int(z_vals[0, 0]), dynamic))
        N, S = sigma_s.shape
        return self.S_.RayMaps(*[torch.zeros(N, 3), torch.zeros(N), torch.zeros(N), torch.zeros(N, S)] * 3, torch.zeros(N))

    def calls(self, name):
        return [e[1:] for e in self.log if e[0] == name]


@pytest.mark.parametrize("late", [False, True])
@pytest.mark.parametrize("dead_work", [False, True])
@pytest.mark.parametrize("name", ["nvidia", "nvidia_no_poses"])
def test_pass_plans_draws_calls_and_counts(name, dead_work, late, monkeypatch):
    """One iteration's passes A-E (and P1-P4 with poses) through step.run_passes, batched and one call per pass: the draws
    (jitter, then a coin unless the pass does not composite, in pass order -- the same in both modes), which field's box
    samples each pass, the passes, colour flag and grad mode of every field call, and what PASSES counts."""
    S_ = pkg("step")
    poses, d = name == "nvidia_no_poses", int(dead_work)
    n_pass = 9 if poses else 5
    dead_rgb = "value" if dead_work else False
    logs = {}
    for batched in (True, False):
        it = _StubIteration(S_, monkeypatch, name, batched, dead_work, 30000 if late else 5000)
        before = collections.Counter(S_.PASSES)
        it.tr.losses(it.batch())
        delta = collections.Counter(S_.PASSES)
        delta.subtract(before)
        assert {k: v for k, v in delta.items() if v} == {k: v for k, v in (
            dict(static=9, static_grad=5, dynamic=4 + 3 * d, dynamic_dead=3 * d) if poses else
            dict(static=5, static_grad=1, dynamic=4 + d, dynamic_dead=d)).items() if v}
        logs[batched] = it
        draws = [e[0] for e in it.log if e[0] in ("jitter", "coin")]
        assert draws == [x for p in PASS_NAMES[:n_pass] for x in (("jitter",) if p in ("P1", "P2") else ("jitter", "coin"))]
        assert it.calls("sample") == [(k, "st" if PASS_NAMES[k] in ("P1", "P2") else "dy") for k in range(n_pass)]
        # every pass but P1 / P2 composites, on the dynamic outputs where a dynamic call ran and on zeros elsewhere
        assert it.calls("composite") == [(k, k < 4 or dead_work) for k in range(n_pass) if PASS_NAMES[k] not in ("P1", "P2")]
    # the order of jitter and coin draws relative to each other, too, is that of the per-pass mode
    assert [e for e in logs[True].log if e[0] in ("jitter", "coin")] == [e for e in logs[False].log if e[0] in ("jitter", "coin")]
    # batched: static A-D cut at the colour flag, dynamic groups by gradient liveness; A-D static under no_grad, E and
    # P1-P4 with grad; a dead dynamic call under no_grad unless its rays require grad (live poses)
    st = [([0, 1, 2, 3], True, False)] if dead_work else [([0], True, False), ([1, 2, 3], False, False)]
    dy = [([0], True, True)] + [(g, dead_rgb, True) for g in ([[1], [2, 3]] if late else [[1, 2, 3]])]
    st += [([4], True, True)]
    dy += [([4], "value", poses)] * d
    if poses:
        st += [([5, 6, 7, 8], dead_rgb, True)]
        dy += [([7, 8], "value", True)] * d
    assert logs[True].calls("st") == st and logs[True].calls("dy") == dy
    # per pass: the same calls cut into single passes (a value-only static call takes "value" as True)
    single = lambda calls: [([k], rgb, grad) for ks, rgb, grad in calls for k in ks]
    assert logs[False].calls("st") == single(st) and logs[False].calls("dy") == single(dy)


def test_image_terms_subset_runs_passes_a_and_e(monkeypatch):
    S_ = pkg("step")
    it = _StubIteration(S_, monkeypatch, "nvidia", True, False, 0)
    capture = {}
    it.tr.losses(it.batch(), terms="image_AE", capture=capture)
    assert [e[0] for e in it.log if e[0] in ("jitter", "coin")] == ["jitter", "coin"] * 2
    assert it.calls("st") == [([0], True, False), ([1], True, True)] and it.calls("dy") == [([0], True, True)]
    assert sorted(capture) == ["A", "E"] and all(type(v) is tuple and len(v) == 4 for v in capture.values())
    assert capture["E"][1] is None and isinstance(capture["A"][2], S_.RayMaps)


def test_ray_pass_is_one_pass_of_the_runner_and_draws_nothing_in_eval(monkeypatch):
    S_ = pkg("step")
    it = _StubIteration(S_, monkeypatch, "nvidia", True, False, 0)
    rays, ts = torch.zeros(N_RAYS, 6), torch.zeros(N_RAYS)
    out = S_.ray_pass(it.tr.st, it.tr.dy, rays, ts, N_SAMPLES, "ndc", it, is_train=False)
    assert it.log == [("sample", 0, "dy"), ("st", [0], True, False), ("dy", [0], True, True), ("composite", 0, True)]
    assert type(out) is tuple and len(out) == 4
    assert isinstance(out[0], S_.FieldOut) and isinstance(out[1], S_.FieldOut) and isinstance(out[2], S_.RayMaps)
    del it.log[:]
    o_s, o_d, outs, xyz = S_.ray_pass(it.tr.st, it.tr.dy, rays, ts, N_SAMPLES, "ndc", it, static_grad=True, rgb_s=False)
    assert it.log == [("jitter",), ("sample", 1, "dy"), ("coin",), ("st", [1], False, True), ("dy", [1], "value", False),
                      ("composite", 1, True)]
    assert o_s.rgb is None and xyz.shape == (N_RAYS, N_SAMPLES, 3)
    assert S_.ray_pass(it.tr.st, it.tr.dy, rays, ts, N_SAMPLES, "ndc", it, static_grad=True, dynamic=False)[1] is None
    assert it.log[-1] == ("composite", 2, False)


def test_field_and_map_tuples_keep_their_slot_order():
    S_ = pkg("step")
    R_ = pkg("renderer")
    F_ = pkg("fields")
    assert S_.FieldOut is F_.FieldOut and S_.RayMaps is R_.RayMaps
    f = F_.FieldOut(*range(10))
    assert tuple(f) == tuple(range(10)) and isinstance(f, tuple)
    assert (f.blending, f.xyz_sampled, f.weight, f.xyz_prime, f.rgb, f.sigma, f.z_vals, f.dists) == tuple(range(2, 10))
    m = R_.RayMaps(*range(13))
    assert tuple(m) == tuple(range(13)) and isinstance(m, tuple)
    assert (m.rgb, m.depth, m.acc, m.weights) == (0, 1, 2, 3) and (m.rgb_s, m.depth_s, m.acc_s, m.weights_s) == (4, 5, 6, 7)
    assert (m.rgb_d, m.depth_d, m.acc_d, m.weights_d) == (8, 9, 10, 11) and m.dynamicness == 12


def test_bench_reads_the_committed_pmc_summaries():
    """bench.py prices `roofline.traffic / hbm_real / l2_atomic_frac` from the committed rocprofv3 summaries under
    profiles/: the parsers must find the scatter family, the dW kernel and the step count in this round's files (a
    silent None would drop the fields from the driver's line)."""
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import bench
    fam = ("void k_scatter<", "void k_scatter_sorted<", "void k_scatter_tiled<")
    fetch = bench.pmc_family_per_step("pmc_fetch", fam, "FETCH_SIZE")
    write = bench.pmc_family_per_step("pmc_write", fam, "WRITE_SIZE")
    atom = bench.pmc_family_per_step("sq_counters", fam, "TCP_TCC_ATOMIC_WITHOUT_RET_REQ_sum")
    assert fetch and write and atom
    assert 1e5 < fetch < 1e7 and 1e5 < write < 1e7          # KB per training step
    assert 1e6 < atom < 1e8                                 # memory-side atomic requests per training step (r05: 6.8 M)
    dw = bench.pmc_traffic("k_dw3")
    assert dw and 1e8 < dw < 1e10                           # bytes per launch
    assert bench._profile_csv("pmc_fetch")[1] == bench.PROFILE_TAG
    # the configuration whose factors exceed the caches: a true HBM fraction of its dominant kernel
    r = bench.committed_hbm_roofline("640_", "640^3")
    assert r and r["bound"] == "hbm" and 0.2 < r["frac"] < 1.0 and 0.2 < r["all_kernels_frac"] < 1.0
    assert r["kernel"].startswith("k_") and r["ms_per_step"] > 1.0


def test_bench_selects_the_baseline_config_of_the_gpu_count():
    """bench.py --gpus N: by default configs[1] (Balloon1, the configuration BASELINE.json's metric is quoted on at 1/2/4/8
    GPUs) at 4096 rays per GPU; --baseline-config quoted selects the configuration quoted for N GPUs:
    N = 4 -> configs[3], DAVIS.txt final grid, 8192 rays global = 2048 per rank; N = 8 -> configs[4], the 640^3 grid, 32768
    rays global = 4096 per rank; explicit flags win."""
    import argparse
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench

    def sel(world, **kw):
        a = argparse.Namespace(config=None, stage=None, baseline_config="auto", rays_per_gpu=0)
        a.__dict__.update(kw)
        b, explicit = bench.select_baseline_config(a, world)
        return b, explicit, a.config, a.stage, a.rays_per_gpu

    for n in (1, 2, 4, 8):   # the metric is quoted on Balloon1 @1/2/4/8: the default at every GPU count (weak scaling)
        assert sel(n) == ("1", False, "nvidia", "stage0", 0)
    assert sel(1, baseline_config="quoted") == ("1", False, "nvidia", "stage0", 0)
    assert sel(4, baseline_config="quoted") == ("3", False, "davis", "final", 2048)
    assert sel(8, baseline_config="quoted") == ("4", False, "nvidia_no_poses", "final", 4096)
    assert sel(8, baseline_config="4") == ("4", False, "nvidia_no_poses", "final", 4096)
    assert sel(4, config="nvidia") == ("1", True, "nvidia", "stage0", 0)
    assert sel(4, rays_per_gpu=512)[4] == 512                       # an explicit per-GPU batch is kept
    assert sel(1, config="davis", stage="stage0")[0] is None        # not a BASELINE configuration


def test_resolution_schedule_matches_the_reference_formulas():
    """step.scene_config("nvidia", stage) for the five stages of configs/Nvidia.txt's schedule: the grids / sample counts are
    those of utils.py:58-65 N_to_reso / cal_n_samples (restated in the oracle) on the log-spaced voxel counts of
    train.py:937-947, and resolution_schedule() covers the 100 000 iterations once."""
    import numpy as np
    import torch
    from oracle import rodynrf_oracle as O
    S_ = pkg("step")
    aabb = torch.tensor(S_.scene_config("nvidia", "stage0")["aabb"])
    nvox = torch.round(torch.exp(torch.linspace(np.log(2097156), np.log(27000000), 5))).long().tolist()
    sched = S_.resolution_schedule("nvidia")
    assert [s[0] for s in sched] == ["stage0", "up1", "up2", "up3", "final"]
    assert sched[0][1] == 0 and sched[-1][2] == 100000 and all(a[2] == b[1] for a, b in zip(sched, sched[1:]))
    assert [s[1] for s in sched[1:]] == [8000, 12000, 16000, 22000]   # configs/Nvidia.txt upsamp_list
    for (stage, first, _), n in zip(sched, nvox):
        cfg = S_.scene_config("nvidia", stage)
        reso = O.N_to_reso(n, aabb)
        assert cfg["grid"] == reso and cfg["n_samples"] == O.cal_n_samples(reso, 2.0), (stage, reso)
        assert cfg["start_iteration"] == (0 if stage == "stage0" else first)


def test_graph_rng_hands_out_the_same_static_slices_every_iteration():
    """GraphRng (Trainer(graph=True)): the draws of an iteration are fixed slices of static memory -- the same storage at
    capture and at every replay -- refilled by begin(); coins are one-element fp32 tensors holding 0 or 1; frozen keeps
    the contents (tests replay fixed draws)."""
    S_ = pkg("step")
    dev = torch.device("cpu")
    r = S_.GraphRng(dev, pool_floats=4096)
    seen = []
    for it in range(3):
        r.begin()
        j = r.jitter(115, "ndc", dev)[0]
        c0, c1 = r.coin(), r.coin()
        jo = r.jitter(221, "contract", dev)
        seen.append((j.data_ptr(), c0.data_ptr(), c1.data_ptr(), jo[0].data_ptr(), jo[1].data_ptr(), j.clone(), float(c0), float(c1)))
        assert j.shape == (115,) and c0.shape == (1,) and c0.dtype == torch.float32
        assert float(c0) in (0.0, 1.0) and float(c1) in (0.0, 1.0)
        assert j.data_ptr() == r.pool[64:].data_ptr()           # the coins' source (pool head) is not handed out as jitter
        assert jo[0].shape[0] == 221 - 221 // 2 + 1 and jo[1].shape[0] == 221 // 2 + 1
        assert torch.equal(r.coins, torch.round(r.pool[:r.N_COINS]))
    assert all(s[:5] == seen[0][:5] for s in seen)             # same addresses every iteration
    assert not torch.equal(seen[0][5], seen[1][5])             # fresh values
    r.frozen = True
    before = r.pool.clone()
    r.begin()
    assert torch.equal(r.pool, before)
    import pytest
    with pytest.raises(RuntimeError):
        for _ in range(r.N_COINS + 1):
            r.coin()
    with pytest.raises(RuntimeError):
        r._take(1 << 20, dev)
