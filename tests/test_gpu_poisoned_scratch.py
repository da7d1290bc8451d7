"""The entry points on hostile scratch.  The saved-row buffers (fields._alloc_saved, fields._feat_saved) and the workspace
(_lib.workspace) are torch.empty: in a long fit() the caching allocator hands back blocks that held indices or images.  k_dw3
and the scatter kernels read whole 32-sample tiles of them (csrc/rdrf_dw.hip, ROW CONTRACT), so every slot a producer leaves
unwritten is a NaN waiting to happen.  Here every such buffer is filled with 0xFF bytes first (a NaN in every float), the
workspace on EVERY call (no entry point may carry state in it from one call to the next), and forward + backward of both
fields, the compositor, the scene flow and the per-point feature entry points run at shapes with ragged tiles everywhere.

Every output and gradient is finite and equals that of the same calls on zero-filled buffers: bit for bit in the deterministic
library; in the product library (fp32 atomics arrive in another order every run) within the convention of
test_tiled_scatter_matches_plain_sorted_scatter_at_benchmark_shape: relative L2 <= max(3 x the run-to-run spread of the
zero-filled path, 2e-6)."""
import contextlib

import pytest
import torch

from _twin import CHILD, run_twin
from _util import pkg, record_margin

pytestmark = pytest.mark.gpu

N, S, GRID, M = 33, 45, (24, 26, 16), 77      # 45 mod 32 = 13: ragged ray tiles; 33 x 45 = 1485: a ragged flat tile array
# (ray type, scatter mode, loss kind, rgb mode of forward()): every value of each at least once
CASES = [("ndc", "ray", "full", True), ("ndc", "sorted", "no_rgb", True), ("ndc", "sorted_plain", "full", "value"),
         ("contract", "sorted", "full", True), ("contract", "ray", "no_rgb", True), ("contract", "sorted_plain", "no_rgb", "value")]
IDS = ["-".join(str(v) for v in c) for c in CASES]


@contextlib.contextmanager
def scratch_fill(byte):
    """every saved-row buffer and every workspace the entry points get is filled with `byte` first"""
    L, F = pkg(), pkg("fields")
    orig = F._alloc_saved, F._feat_saved, L.workspace
    seen = {"saved": 0, "workspace": 0}

    def filled(fn, key):
        def wrapper(*a, **k):
            r = fn(*a, **k)
            buf = r[0] if isinstance(r, tuple) else r
            if buf is not None:
                buf.fill_(byte)
                seen[key] += 1
            return r
        return wrapper

    F._alloc_saved, F._feat_saved, L.workspace = filled(orig[0], "saved"), filled(orig[1], "saved"), filled(orig[2], "workspace")
    try:
        yield seen
    finally:
        F._alloc_saved, F._feat_saved, L.workspace = orig


@pytest.fixture
def poisoned_scratch():
    with scratch_fill(0xFF) as seen:
        yield seen


def _fields(rt, seed=3):
    import rodynrf
    from _gpu_util import COMMON
    L = pkg()
    torch.manual_seed(seed)
    contract = rt == "contract"
    aabb = torch.tensor([[-2.0, -2.0, -2.0], [2.0, 2.0, 2.0]] if contract else [[-1.5, -1.67, -1.0], [1.5, 1.67, 1.0]])
    kw = dict(COMMON, near_far=[0.05, 256.0] if contract else [0.0, 1.0], density_shift=-1.0 if contract else -10.0,
              fea2denseAct="softplus" if contract else "relu")
    st = rodynrf.TensorVMSplit(aabb, list(GRID), 12, "cuda", shadingMode="MLP_Fea_TimeEmbedding" if contract else "MLP_Fea",
                               fea_pe=2, **kw)
    dy = rodynrf.TensorVMSplit_TimeEmbedding(aabb, list(GRID), 12, "cuda", shadingMode="MLP_Fea_late_view", fea_pe=0, **kw)
    if L.DETERMINISTIC:
        st.fused_grad = dy.fused_grad = True
    return st, dy


def _batch(dy, rt):
    import rodynrf
    from _gpu_util import make_rays
    contract = rt == "contract"
    rays, ts = make_rays(N, 14, rt)
    rays, ts = rays.cuda(), ts.cuda()
    jit = torch.rand(S - S // 2 + 1 if contract else S, generator=torch.Generator().manual_seed(4)).cuda()
    extra = {"jitter_outer": torch.rand(S // 2 + 1, generator=torch.Generator().manual_seed(5)).cuda()} if contract else {}
    xyz, z, valid = rodynrf.sampleXYZ(dy, rays, S, ray_type=rt, is_train=True, jitter=jit, **extra)
    valid = valid.bool() & (torch.rand(N, S, generator=torch.Generator().manual_seed(6)).cuda() > 0.2)
    idx = valid.flatten().nonzero().flatten()
    assert len(idx) > 64
    if len(idx) % 32 == 0:      # the compacted count is never a whole number of tiles
        valid.view(-1)[idx[0]] = False
    assert int(valid.sum()) % 32 != 0
    tgt = torch.rand(N, 3, generator=torch.Generator().manual_seed(9)).cuda()
    return rays, ts, xyz.detach(), z.detach(), valid, tgt


def _zero_grads(*fields):
    for f in fields:
        for p in f.parameters():
            if p.grad is not None:
                p.grad.zero_()


def _collect(fields, out):
    for tag, f in zip(("st", "dy"), fields):
        f.det_fold_()
        for k, p in f.named_parameters():
            if p.grad is not None:
                out[f"grad.{tag}.{k}"] = p.grad.detach().clone()
    torch.cuda.synchronize()
    return out


def run_rays(st, dy, batch, rt, mode, loss_kind, rgb):
    """forward + backward of both fields with raw2outputs and scene flow -> {name: tensor} of every output and gradient"""
    import rodynrf
    L = pkg()
    rays, ts, xyz, z, valid, tgt = batch
    _zero_grads(st, dy)
    L.set_scatter_mode(mode)
    try:
        o_s = st(rays, ts, None, xyz, z, valid, is_train=True, ray_type=rt, N_samples=S, rgb=rgb)
        o_d = dy(rays, ts, None, xyz, z, valid, is_train=True, ray_type=rt, N_samples=S, rgb=rgb)
        outs = rodynrf.raw2outputs(o_s[6], o_s[7], o_d[6], o_d[7], o_d[9], o_d[2], o_d[8], rays, is_train=True, ray_type=rt,
                                   add_white_bg=True)
        sf = dy.get_forward_backward_scene_flow(o_d[3], ts)
        rm = lambda x: x.mean()
        if loss_kind == "no_rgb":      # only weights / depths / dynamicness: the appearance heads get no gradient
            loss = 0.1 * rm(outs[12]) + 0.05 * rm(outs[9]) + N * S * rm(outs[11] ** 2) + 0.01 * rm(sf[0] ** 2)
        else:
            loss = (3 * rm((outs[0] - tgt) ** 2) + rm((outs[8] - tgt) ** 2) + rm((outs[4] - tgt) ** 2) + 0.1 * rm(outs[12])
                    + 0.05 * rm(outs[9]) + 0.01 * rm(sf[0] ** 2) + 0.01 * rm(sf[1] ** 2))
        loss.backward()
    finally:
        L.set_scatter_mode("auto")
    res = {"loss": loss.detach().reshape(1)}
    for tag, o in (("st", o_s), ("dy", o_d), ("comp", outs), ("sf", sf)):
        for i, v in enumerate(o):
            if torch.is_tensor(v) and v.is_floating_point():
                res[f"out.{tag}.{i}"] = v.detach().clone()
    return _collect((st, dy), res)


def run_features(st, dy):
    """the per-point entry points at M points, forward + backward"""
    g = torch.Generator().manual_seed(12)
    xn = (torch.rand(M, 3, generator=g) * 1.9 - 0.95).cuda()
    tm = (torch.randint(0, 12, (M,), generator=g).float() * 2 / 11 - 1).cuda()
    w = torch.randn(M, 27, generator=g).cuda()
    _zero_grads(st, dy)
    res = {"s_density": st.compute_densityfeature(xn, tm, None), "s_app": st.compute_appfeature(xn, tm, None),
           "d_density": dy.compute_densityfeature(xn, tm, None), "d_blending": dy.compute_blendingfeature(xn, tm, None),
           "d_app": dy.compute_appfeature(xn, tm, None), "d_warp": dy.warp_coordinate(dy.unnormalize_coord(xn), tm)}
    (res["s_density"].sum() + (res["s_app"] * w).sum() + res["d_density"].sum() + res["d_blending"].sum() + (res["d_app"] * w).sum()
     + (res["d_warp"] * w[:, :3]).sum()).backward()
    return _collect((st, dy), {"out." + k: v.detach().clone() for k, v in res.items()})


def _finite(res, what):
    bad = [k for k, v in res.items() if not bool(torch.isfinite(v).all())]
    assert not bad, f"{what}: not finite under poisoned scratch: {bad}"


def _vec(res, prefix):
    return torch.cat([v.flatten().double() for k, v in sorted(res.items()) if k.startswith(prefix)])


def _compare(poison, zero_a, zero_b, what):
    """bit-equal in the deterministic library; else relative L2 <= max(3 x spread of the zero-filled path, 2e-6), over the
    outputs, over the gradients and for every tensor on its own"""
    L = pkg()
    assert sorted(poison) == sorted(zero_a) == sorted(zero_b)
    assert any(k.startswith("grad.st.") for k in poison) and any(k.startswith("grad.dy.") for k in poison)
    if L.DETERMINISTIC:
        diff = [k for k in poison if not torch.equal(poison[k], zero_a[k])]
        assert not diff, f"{what}: differ from the zero-filled run: {diff}"
        return
    groups = [(prefix, _vec(poison, prefix), _vec(zero_a, prefix), _vec(zero_b, prefix)) for prefix in ("out.", "grad.")]
    groups += [(k, poison[k].flatten().double(), zero_a[k].flatten().double(), zero_b[k].flatten().double()) for k in sorted(poison)]
    worst, bad = 0.0, []
    for name, p, a, b in groups:      # all outputs, all gradients, then every tensor on its own: a small one cannot hide
        nrm = float(a.norm())
        if nrm == 0:
            assert float(p.abs().max()) == 0, (what, name)
            continue
        spread, dist = float((a - b).norm()) / nrm, float((p - a).norm()) / nrm
        bound = max(3 * spread, 2e-6)
        if name in ("out.", "grad."):
            print(f"{what} {name} rel. L2 poisoned vs zero-filled {dist:.3e}, spread {spread:.3e}")
        worst = max(worst, dist / bound)
        if dist > bound:
            bad.append((name, dist, spread))
    record_margin("poisoned vs zero-filled scratch (rel. L2 / max(3 spread, 2e-6), worst tensor)", worst)
    assert not bad, (what, bad)


def _case(rt, mode, loss_kind, rgb):
    st, dy = _fields(rt)
    batch = _batch(dy, rt)
    with scratch_fill(0x00):
        zero_a = run_rays(st, dy, batch, rt, mode, loss_kind, rgb)
        zero_b = run_rays(st, dy, batch, rt, mode, loss_kind, rgb)
    with scratch_fill(0xFF) as seen:
        poison = run_rays(st, dy, batch, rt, mode, loss_kind, rgb)
    assert seen["saved"] >= 3 and seen["workspace"] >= 3, seen      # both fields and the scene flow
    return poison, zero_a, zero_b


@pytest.mark.parametrize("rt,mode,loss_kind,rgb", CASES, ids=IDS)
def test_fields_on_poisoned_scratch(rt, mode, loss_kind, rgb):
    what = f"{rt} {mode} {loss_kind} rgb={rgb}"
    poison, zero_a, zero_b = _case(rt, mode, loss_kind, rgb)
    _finite(poison, what)
    _compare(poison, zero_a, zero_b, what)


def test_feature_entry_points_on_poisoned_scratch(poisoned_scratch):
    st, dy = _fields("ndc")
    poison = run_features(st, dy)
    assert poisoned_scratch["saved"] >= 2 and poisoned_scratch["workspace"] >= 2, poisoned_scratch
    with scratch_fill(0x00):      # the inner patch wraps the poisoning one: the zero fill comes last
        zero_a, zero_b = run_features(st, dy), run_features(st, dy)
    _finite(poison, f"features M = {M}")
    _compare(poison, zero_a, zero_b, f"features M = {M}")


def test_poisoned_scratch_changes_no_bit_in_the_deterministic_library(tmp_path):
    """the same cases against librodynrf_det.so in a child process (the library is chosen at import): every tensor bit for bit"""
    assert run_twin(tmp_path, [CHILD, "poison"], det=True) == len(CASES) + 1
