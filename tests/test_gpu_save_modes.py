"""Rows are saved only where a backward can read them: a field call under torch.no_grad() keeps
nothing, forward(rgb="value") computes the colours but saves no appearance rows (RDRF_SAVE_NO_APP), the backward entry
points refuse a colour gradient for such a buffer, and the trainer's dead work saves accordingly -- with every output,
loss and gradient what it was.  Shapes: 70 rays x 13 / 45 samples of the ndc_relu / contract_relu_te cases (910 / 3150
samples: no multiple of 32, rays cross tile edges, the last tile is ragged).

Under RDRF_DETERMINISTIC=1 (librodynrf_det.so) the gradient comparisons are bitwise; the last test re-runs them there."""
import ctypes as C
import functools
import os
import subprocess
import sys

import pytest
import torch

from _util import assert_close, pkg, record_margin

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 70
CASES = ["ndc_relu", "contract_relu_te"]
SHAPES = [(c, s) for c in CASES for s in (13, 45)]
# outputs of the 10-tuple that stay differentiable when the colours are values only
LIVE = {"static": (7, 4), "dynamic": (2, 4, 5, 7)}


@functools.lru_cache(maxsize=None)
def _fields(case):
    from _gpu_util import fields_from_case
    g, st, dy, _ = fields_from_case(case)
    return str(g["meta.ray_type"]), {"static": st, "dynamic": dy}


@functools.lru_cache(maxsize=None)
def _inputs(case, S):
    """(ray type, fields, (rays, ts, xyz, z, valid)): computed once per shape, shared by the tests, never modified"""
    import rodynrf
    from _gpu_util import make_rays
    rt, fields = _fields(case)
    rays, ts = (t.cuda() for t in make_rays(N, 3, rt))
    with torch.no_grad():
        xyz, z, valid = rodynrf.sampleXYZ(fields["dynamic"], rays, S, ray_type=rt, is_train=False)
    return rt, fields, (rays, ts, xyz, z, valid)


def _call(field, rt, inp, rgb=True, leaf=False):
    rays, ts, xyz, z, valid = inp
    if leaf:
        xyz, z = xyz.clone().requires_grad_(True), z.clone().requires_grad_(True)
    return field(rays, ts, None, xyz, z, valid, is_train=True, ray_type=rt, rgb=rgb), xyz, z


def _assert_outputs_bit_equal(a, b, what):
    assert [v is None for v in a] == [v is None for v in b], what
    for i, (x, y) in enumerate(zip(a, b)):
        if x is not None:
            assert torch.equal(x.detach(), y.detach()), f"{what}: entry {i} of the 10-tuple differs"


@pytest.mark.parametrize("kind", ["static", "dynamic"])
@pytest.mark.parametrize("case,S", SHAPES)
def test_no_grad_forward_saves_nothing_and_returns_the_same_bits(case, S, kind):
    """A field call under torch.no_grad() with parameters that require grad (ctx.needs_input_grad says True there): every
    output bit-equal to the grad-mode call, and the allocation peak rises over the call by less than the saved buffer the
    call used to allocate; the grad-mode call, measured the same way, rises by at least that buffer."""
    F, L = pkg("fields"), pkg()
    rt, fields, inp = _inputs(case, S)
    field = fields[kind]
    assert all(p.requires_grad for p in field.parameters())
    saved_bytes = int(L.lib.rdrf_saved_bytes(1 if kind == "dynamic" else 0, N, S))

    def rise(grad):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.max_memory_allocated()
        F.SAVE_STATS.clear()
        with torch.set_grad_enabled(grad):
            o, _, _ = _call(field, rt, inp)
        torch.cuda.synchronize()
        return o, torch.cuda.max_memory_allocated() - before, dict(F.SAVE_STATS)

    o_g, rise_g, stats_g = rise(True)    # (also sizes the cached workspace for both modes)
    o_n, rise_n, stats_n = rise(False)
    print(f"{case} S={S} {kind}: saved buffer {saved_bytes} B, peak rise grad mode {rise_g} B, no_grad {rise_n} B")
    _assert_outputs_bit_equal(o_n, o_g, f"{kind} no_grad vs grad mode")
    assert not any(v.requires_grad for v in o_n if v is not None)
    assert rise_g >= saved_bytes
    assert rise_n < saved_bytes, (rise_n, saved_bytes)
    k = 1 if kind == "dynamic" else 0
    assert stats_g == {(k, "full"): 1, (k, "bytes"): saved_bytes} and stats_n == {(k, "none"): 1}


def _grads(field, kind, rt, inp, rgb, gouts):
    """(outputs, flat parameter gradient, g_xyz, g_z) of loss = sum <out_k, g_k> over the outputs LIVE[kind]"""
    field.fused_grad = True
    field.zero_grad_fused()
    o, xyz, z = _call(field, rt, inp, rgb=rgb, leaf=True)
    sum((o[k] * g).sum() for k, g in zip(LIVE[kind], gouts)).backward()
    field.det_fold_()
    torch.cuda.synchronize()
    return o, field._gflat.detach().clone(), xyz.grad.detach().clone(), z.grad.detach().clone()


@pytest.mark.parametrize("kind", ["static", "dynamic"])
@pytest.mark.parametrize("case,S", SHAPES)
def test_value_rgb_changes_no_output_and_no_gradient(case, S, kind):
    """forward(rgb="value"): every output bit-equal to rgb=True, the colours not differentiable, the saved buffer without
    its appearance block; backward of a loss on the remaining outputs (static: sigma, weight; dynamic: blending, weight,
    xyz_prime, sigma): parameter gradients, g_xyz and g_z bit-equal to the rgb=True run in the deterministic library; in
    the product library (fp32 atomics arrive in another order every run) within 3 x the run-to-run spread of two rgb=True
    runs, floor 2e-6 relative L2 -- the convention of test_tiled_scatter_matches_plain_sorted_scatter_at_benchmark_shape."""
    F, L = pkg("fields"), pkg()
    rt, fields, inp = _inputs(case, S)
    field = fields[kind]
    k = 1 if kind == "dynamic" else 0
    gen = torch.Generator().manual_seed(11)
    with torch.no_grad():
        shapes = [None if v is None else v.shape for v in _call(field, rt, inp)[0]]
    gouts = [torch.randn(shapes[i], generator=gen).cuda() for i in LIVE[kind]]
    try:
        o_a, *g_a = _grads(field, kind, rt, inp, True, gouts)
        o_b, *g_b = _grads(field, kind, rt, inp, True, gouts)
        F.SAVE_STATS.clear()
        o_v, *g_v = _grads(field, kind, rt, inp, "value", gouts)
        stats = dict(F.SAVE_STATS)
    finally:
        field.fused_grad = False
        for p in field.parameters():
            p.grad = None
    assert stats == {(k, "no_app"): 1, (k, "bytes"): int(L.lib.rdrf_saved_bytes_ex(k, N, S, L.SAVE_NO_APP))}
    _assert_outputs_bit_equal(o_v, o_a, f"{kind} rgb='value' vs rgb=True")
    assert o_a[6].requires_grad and not o_v[6].requires_grad
    assert all(o_v[i].requires_grad for i in LIVE[kind])
    for name, a, b, v in zip(("parameters", "g_xyz", "g_z"), g_a, g_b, g_v):
        nrm = float(a.double().norm())
        if name == "g_z" and nrm == 0.0:   # (no path from these outputs to z_vals for this ray type)
            assert not bool(v.any())
            continue
        assert nrm > 0, name
        if L.DETERMINISTIC:
            assert torch.equal(v, a), f"{name}: rgb='value' changed the gradient bits in the deterministic build"
            continue
        spread = float((a.double() - b.double()).norm()) / nrm
        dist = float((v.double() - a.double()).norm()) / nrm
        print(f"{case} S={S} {kind} {name}: rel. L2 distance {dist:.3e}, run-to-run spread {spread:.3e}")
        record_margin(f"rgb='value' vs rgb=True {name} (rel. L2 / max(3 spread, 2e-6))", dist / max(3 * spread, 2e-6))
        assert dist <= max(3 * spread, 2e-6), (name, dist, spread)


@pytest.mark.parametrize("kind", ["static", "dynamic"])
@pytest.mark.parametrize("case,S", SHAPES)
def test_backward_refuses_a_colour_gradient_for_a_buffer_without_appearance_rows(case, S, kind):
    """C ABI: rdrf_saved_bytes_ex(RDRF_SAVE_NO_APP) is the full size minus the appearance block; rdrf_*_bwd given such a
    buffer and a non-NULL g_rgb returns a negative code with a message and touches no gradient output (pre-filled with a
    sentinel); half of that buffer is refused as too small; the same buffer without g_rgb differentiates."""
    F, L = pkg("fields"), pkg()
    rt, fields, inp = _inputs(case, S)
    field = fields[kind]
    dyn = kind == "dynamic"
    rays, ts, xyz, z, valid = inp
    valid8 = valid.contiguous().view(torch.uint8) if valid.dtype == torch.bool else valid.contiguous()
    dev = z.device
    tiles = (N * S + 31) // 32
    full = int(L.lib.rdrf_saved_bytes(int(dyn), N, S))
    nbytes = int(L.lib.rdrf_saved_bytes_ex(int(dyn), N, S, L.SAVE_NO_APP))
    assert nbytes == full - (tiles * 32 * int(L.lib.rdrf_saved_row_bytes(1 if dyn else 2)) + 256)
    params = [p.detach() for p in field._param_list()]
    struct = F._dynamic_struct if dyn else F._static_struct
    P, cfg = struct(params), F._cfg_struct(field, rt)
    saved = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    ws = L.workspace(dev, L.lib.rdrf_workspace_bytes(N, S))
    out = {k: torch.empty(N, S, device=dev) for k in ("sigma", "weight", "dists", "blending")}
    rgb, xyz_prime = torch.empty(N, S, 3, device=dev), torch.empty(N, S, 3, device=dev)
    head = (C.byref(P), C.byref(cfg), L.ptr(rays), L.ptr(ts), L.ptr(xyz), L.ptr(z), L.ptr(valid8), N, S)
    tail = (L.ptr(ws), C.c_size_t(ws.numel()), L.stream_of(z))
    if dyn:
        rc = L.lib.rdrf_dynamic_fwd_ex(*head, L.ptr(out["blending"]), L.ptr(out["weight"]), L.ptr(xyz_prime), L.ptr(rgb),
                                       L.ptr(out["sigma"]), L.ptr(out["dists"]), L.ptr(saved), C.c_size_t(nbytes), *tail,
                                       L.SAVE_NO_APP)
    else:
        rc = L.lib.rdrf_static_fwd_ex(*head, L.ptr(rgb), L.ptr(out["sigma"]), L.ptr(out["weight"]), L.ptr(out["dists"]),
                                      L.ptr(saved), C.c_size_t(nbytes), *tail, L.SAVE_NO_APP)
    L.check(rc, "forward with RDRF_SAVE_NO_APP")
    torch.cuda.synchronize()
    with torch.no_grad():
        ref = _call(field, rt, inp)[0]
    assert torch.equal(rgb, ref[6]) and torch.equal(out["weight"], ref[4]) and torch.equal(out["sigma"], ref[7])

    SENT = 7.0
    grads = [torch.full_like(p, SENT) for p in params]
    G = struct(grads)
    g_xyz, g_z, g_rays = torch.full_like(xyz, SENT), torch.full_like(z, SENT), torch.full_like(rays, SENT)
    g_rgb, g_sigma = torch.ones(N, S, 3, device=dev), torch.ones(N, S, device=dev)

    def bwd(g_rgb_, g_sigma_, bytes_):
        gtail = (C.byref(G), L.ptr(g_xyz), L.ptr(g_z), L.ptr(g_rays), L.ptr(saved), C.c_size_t(bytes_), *tail)
        if dyn:   # g_blending, g_weight, g_xyz_prime, g_rgb, g_sigma, g_dists
            rc_ = L.lib.rdrf_dynamic_bwd(*head, None, None, None, L.ptr(g_rgb_), L.ptr(g_sigma_), None, *gtail)
        else:     # g_rgb, g_sigma, g_weight, g_dists
            rc_ = L.lib.rdrf_static_bwd(*head, L.ptr(g_rgb_), L.ptr(g_sigma_), None, None, *gtail)
        torch.cuda.synchronize()
        return rc_, L.lib.rdrf_last_error().decode()

    untouched = lambda: all(bool((t == SENT).all()) for t in grads + [g_xyz, g_z, g_rays])
    rc, msg = bwd(g_rgb, g_sigma, nbytes)
    assert rc < 0 and "RDRF_SAVE_NO_APP" in msg and "rgb" in msg, (rc, msg)
    assert untouched(), "a refused backward wrote a gradient"
    rc, msg = bwd(None, g_sigma, nbytes // 2)
    assert rc < 0 and "too small" in msg, (rc, msg)
    assert untouched(), "a refused backward wrote a gradient"
    rc, msg = bwd(None, g_sigma, nbytes)
    assert rc == 0, (rc, msg)
    assert not untouched(), "the density backward of a no-app buffer wrote nothing"


SMALL_NVIDIA = dict(grid=[24, 26, 16], n_samples=24, batch_size=64, H=27, W=48, T=6)   # SMALL["nvidia"] of test_gpu_trainer.py


@pytest.mark.parametrize("it", [0, 30000])
def test_trainer_dead_work_saves_only_what_a_backward_reads(it):
    """Toy grid, 64 rays, stage 0 and a late iteration: a step with dead_work=True gives the loss and the flat gradients
    of dead_work=False -- bitwise in the deterministic library, within the bounds of
    test_dead_work_pruning_changes_nothing in the product one -- and its forwards save (fields.SAVE_STATS, the
    saved-byte accounting of every field call): nothing for the value-only static call of passes A-D nor for the dead
    dynamic forward of pass E, no appearance rows for the dynamic passes B-D, full rows for pass A (dynamic) and pass E
    (static) alone."""
    F, L = pkg("fields"), pkg()
    S_ = pkg("step")
    cfg = S_.scene_config("nvidia", "stage0")
    cfg.update(SMALL_NVIDIA)
    cfg["focal"] = max(cfg["H"], cfg["W"]) / 2.0 * 3.0 ** 0.5
    dev = torch.device("cuda", 0)
    n, s = cfg["batch_size"], cfg["n_samples"]
    got, stats, passes = {}, {}, {}
    for dead in (True, False):
        tr = S_.Trainer(dict(cfg), dev, dead_work=dead)
        tr.it = it
        F.SAVE_STATS.clear()
        before = dict(S_.PASSES)
        tr.step()
        torch.cuda.synchronize()
        stats[dead] = dict(F.SAVE_STATS)
        passes[dead] = {k: v - before.get(k, 0) for k, v in S_.PASSES.items()}
        got[dead] = ([v.detach().clone() for v in tr.last.values()], [g.detach().clone() for g in tr.grad_flats])
    for a, b in zip(got[True][0], got[False][0]):
        if L.DETERMINISTIC:
            assert torch.equal(a, b), "loss"
        else:
            assert_close(a, b, "loss", rtol=1e-6)
    for a, b in zip(got[True][1], got[False][1]):
        assert float(a.abs().max()) > 0
        if L.DETERMINISTIC:
            assert torch.equal(a, b), "dead work changed the gradient bits in the deterministic build"
        else:
            rel = float((a - b).norm() / a.norm())
            print(f"it={it}: dead_work True vs False gradient rel. L2 {rel:.3e}")
            assert rel < 1e-5, rel
    st = stats[True]
    print(f"it={it}: SAVE_STATS with dead_work=True {st}")
    assert passes[True] == dict(static=5, static_grad=1, dynamic=5, dynamic_dead=1)
    late = it >= cfg["upsamp_list"][3]   # passes B-D: one batched dynamic call early, B | C + D late
    sb = lambda kind, rays, flags=0: int(L.lib.rdrf_saved_bytes_ex(kind, rays, s, flags))
    # static: the 4 N-ray value-only call of passes A-D keeps nothing -- pass E is the only call with rows
    assert st[(0, "none")] == 1 and st[(0, "full")] == 1 and (0, "no_app") not in st
    assert st[(0, "bytes")] == sb(0, n)
    # dynamic: pass A full, passes B-D without appearance rows, the dead forward of pass E nothing
    assert st[(1, "full")] == 1 and st[(1, "none")] == 1 and st[(1, "no_app")] == (2 if late else 1)
    no_app = sb(1, n, L.SAVE_NO_APP) + sb(1, 2 * n, L.SAVE_NO_APP) if late else sb(1, 3 * n, L.SAVE_NO_APP)
    assert st[(1, "bytes")] == sb(1, n) + no_app
    assert st[(2, "full")] == 1
    assert not any(mode == "no_app" for _, mode in stats[False])


def test_gradients_are_bitwise_unchanged_in_the_deterministic_build():
    """the gradient comparisons of this file against librodynrf_det.so (fixed-point accumulation: nothing depends on the
    order of arrival), where they are bitwise: 8 field cases + 2 trainer steps"""
    env = dict(os.environ, RDRF_DETERMINISTIC="1")
    env.pop("RDRF_LIB", None)
    env.pop("RDRF_MARGINS", None)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-p", "no:cacheprovider",
                        "-k", "test_value_rgb_changes_no_output_and_no_gradient or test_trainer_dead_work_saves_only"],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "10 passed" in r.stdout, (r.stdout[-3000:], r.stderr[-2000:])
