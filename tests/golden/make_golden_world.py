"""Golden vectors of the WORLD-space ray path (every ray_type but "ndc" / "contract": TensorBase.sample_ray, the `else`
branch of TensorBase.forward and the raw2outputs branch without a far-plane depth term), made by importing the REFERENCE
itself exactly as make_golden.py does (same stubs, same CPU get_device shim).  Data only:

    tests/golden/world.npz          rays (built by construction, see build_rays), times, per-ray jitter, sample_ray in eval and
                                    train mode at S = 33 and 70, the forward tuples of both fields and the 13 outputs of
                                    raw2outputs for two configurations, the loss weights, the loss and d loss / d rays
    tests/golden/world_weights.npz  the state_dicts of the two fields (shared by both configurations)
    tests/golden/world_grads.npz    d loss / d parameter for every parameter of both fields

(three files because the weights and their gradients alone are 1.5 MB and no committed file may exceed 1 MiB)

    python tests/golden/make_golden_world.py
"""
import os

import numpy as np
import torch

from make_golden import HERE, build_fields, import_reference, to_np

GRID = [17, 19, 11]
AABB = [[-1.2, -0.7, 0.3], [1.6, 1.1, 2.1]]     # 2.8 x 1.8 x 1.8, centre (0.2, 0.2, 1.2)
NEAR_FAR = [0.5, 4.0]
STEP_RATIO = 0.5
N = 67
SAMPLES = (33, 70)
# (tag, activation, density_shift, S, train-mode sampler): the first carries the gradients
CONFIGS = (("a", "softplus", -1.0, 33, True), ("b", "relu", -10.0, 70, False))
NAMES = ["_0", "_1", "blending", "pts_ref", "weight", "xyz_prime", "rgb", "sigma", "z", "dists"]
ONAMES = ["rgb_map_full", "depth_map_full", "acc_map_full", "weights_full", "rgb_map_s", "depth_map_s", "acc_map_s",
          "weights_s", "rgb_map_d", "depth_map_d", "acc_map_d", "weights_d", "dynamicness_map"]


def build_rays():
    """67 rays by construction; kind[n]: 0-5 enters through face lo/hi of axis kind // 2 (kind % 2: 0 lo, 1 hi) with the clamp
    inactive, 6 starts inside the box (t_min clamps to near), 7 enters beyond far (t_min clamps to far), 8 misses the box,
    9 axis-parallel (one direction component exactly 0)."""
    g = torch.Generator().manual_seed(20240917)
    lo, hi = torch.tensor(AABB[0]), torch.tensor(AABB[1])
    near, far = NEAR_FAR
    U = lambda a, b, *s: torch.empty(*s).uniform_(a, b, generator=g)
    rays, kind = [], []

    def through_face(axis, upper, t_entry, scale, zero=None):
        p = lo + (hi - lo) * U(0.15, 0.85, 3)
        p[axis] = hi[axis] if upper else lo[axis]
        d = U(0.15, 0.6, 3) * torch.where(U(0, 1, 3) < 0.5, -1.0, 1.0)
        d[axis] = (-1.0 if upper else 1.0) * float(U(0.7, 1.0, 1))     # inward, and the steepest component
        if zero is not None:
            d[zero] = 0.0
        d = d * scale
        return torch.cat([p - d * t_entry, d])

    for face in range(6):                       # (a) every face, clamp inactive
        for _ in range(8 if face < 4 else 7):
            rays.append(through_face(face // 2, face % 2 == 1, float(U(near + 0.3, far - 0.5, 1)), float(U(0.4, 1.2, 1))))
            kind.append(face)
    for _ in range(8):                          # (b) origin inside the box
        o = lo + (hi - lo) * U(0.2, 0.8, 3)
        d = U(0.2, 1.0, 3) * torch.where(U(0, 1, 3) < 0.5, -1.0, 1.0) * float(U(0.4, 1.0, 1))
        rays.append(torch.cat([o, d]))
        kind.append(6)
    for i in range(4):                          # the other side of the clamp: the box begins beyond far
        rays.append(through_face(i % 3, i % 2 == 0, float(U(far + 0.4, far + 1.0, 1)), float(U(0.5, 1.0, 1))))
        kind.append(7)
    for i in range(4):                          # (c) past the box: aimed at a point 0.4-0.9 outside one slab
        axis = i % 3
        q = lo + (hi - lo) * U(0.2, 0.8, 3)
        q[axis] = (hi[axis] + float(U(0.4, 0.9, 1))) if i % 2 else (lo[axis] - float(U(0.4, 0.9, 1)))
        d = U(0.3, 0.9, 3) * torch.where(U(0, 1, 3) < 0.5, -1.0, 1.0)
        d[axis] = d[axis] * 0.05                # nearly parallel to that slab: never crosses into it inside the march
        rays.append(torch.cat([q - d * float(U(1.0, 3.0, 1)), d]))
        kind.append(8)
    for i in range(5):                          # (e) one component exactly 0 (the origin inside that slab)
        axis = i % 3
        rays.append(through_face(axis, i % 2 == 0, float(U(near + 0.3, far - 0.5, 1)), float(U(0.5, 1.0, 1)),
                                 zero=(axis + 1 + i % 2) % 3))
        kind.append(9)
    rays, kind = torch.stack(rays), torch.tensor(kind)
    assert rays.shape == (N, 6)
    return rays, kind


def check_rays(rays, kind, near, far):
    """the conditions of the fixture, in float64: no two axes tie for t_min, t_min is not within 1e-3 of near / far unless
    clamped on purpose, every kind is what it says"""
    r = rays.double()
    lo, hi = torch.tensor(AABB[0]).double(), torch.tensor(AABB[1]).double()
    vec = torch.where(r[:, 3:] == 0, torch.full_like(r[:, 3:], 1e-6), r[:, 3:])
    ra, rb = (hi - r[:, :3]) / vec, (lo - r[:, :3]) / vec
    m = torch.minimum(ra, rb)
    top = m.sort(-1, descending=True)[0]
    assert float((top[:, 0] - top[:, 1]).min()) > 1e-3, "two axes tie for t_min"
    raw, axis = m.max(-1)
    assert float((raw - near).abs().min()) > 1e-3 and float((raw - far).abs().min()) > 1e-3
    upper = ra.gather(1, axis[:, None])[:, 0] < rb.gather(1, axis[:, None])[:, 0]
    for face in range(6):
        sel = kind == face
        assert bool(((axis[sel] == face // 2) & (upper[sel] == (face % 2 == 1)) & (raw[sel] > near) & (raw[sel] < far)).all())
        assert int(sel.sum()) >= 3
    assert bool((raw[kind == 6] < near).all()) and bool((raw[kind == 7] > far).all())
    assert int((kind == 8).sum()) >= 3 and bool(((rays[kind == 9, 3:] == 0).sum(-1) == 1).all())
    return raw, axis


def main():
    TS, TD, renderer, _, _ = import_reference()
    aabb = torch.tensor(AABB)
    rays0, kind = build_rays()
    check_rays(rays0, kind, *NEAR_FAR)
    g = torch.Generator().manual_seed(11)
    ts = torch.randint(0, 12, (N,), generator=g).float() * 2 / 11 - 1
    out = {"meta.grid": np.array(GRID), "meta.near_far": np.array(NEAR_FAR, dtype=np.float32),
           "meta.step_ratio": np.array(STEP_RATIO, dtype=np.float32), "meta.static_head": np.array("MLP_Fea"),
           "aabb": aabb.numpy(), "rays": rays0.numpy(), "kind": kind.numpy(), "ts": ts.numpy()}
    fields = {}
    for tag, act, shift, S, train in CONFIGS:
        st, dy = build_fields(TS, TD, aabb, GRID, act, "MLP_Fea", shift, 20240918)    # one seed: the same weights
        for m in (st, dy):
            m.near_far = list(NEAR_FAR)
            m.step_ratio = STEP_RATIO
            m.update_stepSize(GRID, 12)
        fields[tag] = (st, dy)
        out[f"{tag}.act"], out[f"{tag}.density_shift"] = np.array(act), np.array(shift, dtype=np.float32)
        out[f"{tag}.S"], out[f"{tag}.train"] = np.array(S), np.array(train)
    st, dy = fields["a"]
    out["meta.stepSize"] = dy.stepSize.numpy()
    for k, v in fields["b"][1].state_dict().items():
        assert torch.equal(v, dy.state_dict()[k]), k

    # ---- sample_ray (models/tensorBase.py:501-522), eval and train, both sample counts; the jitter is the [N,1] draw of
    # rand_like(rng[:, [0]]), reproduced by replaying the generator
    torch.manual_seed(5150)
    u = torch.rand(N, 1)
    out["u"] = u[:, 0].numpy()
    smp = {}
    for S in SAMPLES:
        for mode, train in (("eval", False), ("train", True)):
            torch.manual_seed(5150)
            xyz, z, valid = dy.sample_ray(rays0[:, :3], rays0[:, 3:], is_train=train, N_samples=S)
            assert z.shape == (N, S) and xyz.shape == (N, S, 3)
            smp[(S, train)] = (xyz, z, valid)
            pre = f"{mode}{S}."
            out[pre + "xyz"], out[pre + "z"], out[pre + "valid"] = xyz.numpy(), z.numpy(), valid.numpy()
            frac = float(valid.float().mean())
            assert 0.25 <= frac <= 0.75, (S, mode, frac)
            assert not bool(valid[kind == 8].any()), "a ray meant to miss the box has a valid sample"
            inside = valid[kind < 6]
            trailing = int((inside[:, 0] & ~inside[:, -1]).sum())
            assert trailing >= 6, "rays that leave the box before the last sample"
            print(f"sample_ray S={S} {mode}: valid {frac:.3f}, entering rays with a trailing invalid run {trailing}")
    allv = torch.cat([v[2].reshape(-1) for v in smp.values()]).float().mean()
    assert 0.25 <= float(allv) <= 0.75

    # ---- forward of both fields and raw2outputs on sample_ray's own output (sampleXYZ tiles the per-ray z_vals, which
    # fails for N > 1: the three stages are called directly)
    for tag, act, shift, S, train in CONFIGS:
        st, dy = fields[tag]
        rays = rays0.clone().requires_grad_(True)
        torch.manual_seed(5150)
        xyz, z, valid = dy.sample_ray(rays[:, :3], rays[:, 3:], is_train=train, N_samples=S)
        ref = smp[(S, train)]
        assert torch.equal(xyz.detach(), ref[0]) and torch.equal(z.detach(), ref[1]) and torch.equal(valid, ref[2])
        kw = dict(is_train=True, white_bg=True, ray_type="world", N_samples=S)
        o_s = st(rays, ts, None, xyz, z, valid, **kw)
        o_d = dy(rays, ts, None, xyz, z, valid, **kw)
        for pre, o in (("fs.", o_s), ("fd.", o_d)):
            assert torch.equal(o[3], xyz) and torch.equal(o[8], z)       # pts_ref / z_vals: the inputs, not stored again
            for k, v in zip(NAMES, o):
                if v is not None and k not in ("pts_ref", "z"):
                    out[f"{tag}.{pre}{k}"] = v.detach().numpy()

        def comp(is_train, want_white):
            sd_ = 0
            while is_train:
                torch.manual_seed(sd_)
                if (torch.rand((1,)) < 0.5).item() == want_white:
                    break
                sd_ += 1
            torch.manual_seed(sd_)
            return renderer.raw2outputs(o_s[6], o_s[7], o_d[6], o_d[7], o_d[9], o_d[2], o_d[8], rays, is_train=is_train,
                                        ray_type="world")

        c_eval, c1 = comp(False, False), comp(True, True)
        for k, a, c in zip(ONAMES, c_eval, c1):
            out[f"{tag}.ce.{k}"], out[f"{tag}.c1.{k}"] = a.detach().numpy(), c.detach().numpy()
        miss = kind == 8
        for k in (0, 1, 2, 4, 5, 6, 8, 9, 10):
            assert float(c_eval[k][miss].abs().max()) == 0.0, ONAMES[k]
        print(f"config {tag} ({act}, S={S}, train={train}): valid {float(valid.float().mean()):.3f} app_mask_d "
              f"{float((o_d[4] > 1e-4).float().mean()):.3f} app_mask_s {float((o_s[4] > 1e-4).float().mean()):.3f} "
              f"acc_full max {float(c_eval[2].max()):.3f}")
        if tag != "a":
            continue
        # ---- one scalar loss over the chain: every output of raw2outputs (train mode, white background) and the fields'
        # own outputs, fixed random weights; gradients wrt the rays and every parameter.  The weights are POSITIVE, uniform in
        # (0.5, 1.5): under signed (normal) weights the one-element gradient of density_layer2.bias is a cancelling sum of
        # ~1500 per-sample terms that the reference itself only defines to 3e-4 of its value -- its own fp32 result moves by
        # that much when nothing but the order of the rays changes -- while every 1e-4 check against it needs a reference
        # that is good to well below 1e-4; with positive weights the same experiment moves no gradient tensor by more than
        # 2e-6 of its max
        gl = torch.Generator().manual_seed(77)
        L = 0.0
        for k, v in zip(ONAMES, c1):
            r = torch.rand(v.shape, generator=gl) + 0.5
            out["lw.c1." + k] = r.numpy()
            L = L + (v * r).sum()
        for k, v in (("blending", o_d[2]), ("weight", o_d[4]), ("xyz_prime", o_d[5]), ("weight_s", o_s[4])):
            r = torch.rand(v.shape, generator=gl) + 0.5
            out["lw.f." + k] = r.numpy()
            L = L + (v * r).sum()
        out["loss"] = L.detach().numpy()
        ps, pd = list(st.parameters()), list(dy.parameters())
        grads = torch.autograd.grad(L, ps + pd + [rays], allow_unused=True)
        gout = {}
        for (k, _), gv in zip(st.named_parameters(), grads[: len(ps)]):
            gout["gs." + k] = (gv if gv is not None else torch.zeros(())).numpy()
        for (k, _), gv in zip(dy.named_parameters(), grads[len(ps): len(ps) + len(pd)]):
            gout["gd." + k] = (gv if gv is not None else torch.zeros(())).numpy()
        out["g.rays"] = grads[-1].numpy()
        np.savez_compressed(os.path.join(HERE, "world_grads.npz"), **gout)
        print(f"loss {float(L.detach()):.5f} |g.rays| {float(grads[-1].abs().max()):.3e}")

    w = {}
    to_np(st.state_dict(), "s.", w)
    to_np(dy.state_dict(), "d.", w)
    np.savez_compressed(os.path.join(HERE, "world_weights.npz"), **w)
    np.savez_compressed(os.path.join(HERE, "world.npz"), **out)
    for f in ("world.npz", "world_weights.npz", "world_grads.npz"):
        size = os.path.getsize(os.path.join(HERE, f))
        assert size < (1 << 20), (f, size)
        print(f, size, "bytes")


if __name__ == "__main__":
    main()
