"""Fixtures of the evaluation render's motion maps: tests/golden/motion_{ndc,contract}.npz.

Runs only where the reference is available (it is imported through make_golden.import_reference; nothing of it is
copied).  Per ray type a 24 x 16 image is pushed through the reference's own per-frame chain in the order of its
`render` (renderer.py:405-537): sampleXYZ -> tensorf_static -> tensorf -> raw2outputs ->
get_forward_backward_scene_flow -> induce_flow x 4 -> the weights_d-weighted sum of delta_xyz (:460, :610), and
flow_viz.flow_to_image of each flow.  Stored: both fields' weights (the layout tests/_gpu_util.fields_from_case reads),
rays, ts, focal, the neighbour poses, the maps, and the flow pictures with their input flows.

The weights are conditioned so that the fixture exercises what it is for, and the generator asserts it:
  * the dynamic density head's output bias is raised until at least half of the rays have sum weights_d > 0.1
  * the scene-flow MLP's last layer is scaled until the dynamic flows differ from the static ones by >= 1 pixel (median)
  * the warp displaces: max |delta_xyz| > 1e-3
  * the reference's fp32 chain lies within 2e-5 max|ref| of the same chain in fp64 (so a 1e-4 comparison against this
    fixture is a statement about the code under test, not about the conditioning of the case)

    python tests/golden/make_golden_motion.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402

H, W, S, T = 16, 24, 40, 12
MAPS = ("flow_f", "flow_b", "flow_s_f", "flow_s_b", "delta_xyz")
DENSITY_BIAS_STEP = 0.25      # added to density_layer2.bias until the dynamic weights carry the rays
SCENE_FLOW_SCALE_STEP = 2.0   # factor on scene_flow_mlp[6] until the dynamic flows leave the static ones


def chain(R, st, dy, rays, ts, grid2d, focal, pose_f, pose_b, ray_type):
    """the per-chunk body of the reference's render (renderer.py:405-537) + the delta_xyz sum (:610), one chunk"""
    xyz, z, valid = R.sampleXYZ(dy, rays, N_samples=S, ray_type=ray_type, is_train=False)
    o_s = st(rays, ts, None, xyz, z, valid, is_train=False, white_bg=True, ray_type=ray_type, N_samples=S)
    o_d = dy(rays, ts, None, xyz, z, valid, is_train=False, white_bg=True, ray_type=ray_type, N_samples=S)
    pts_ref_s, rgb_s, sigma_s = o_s[3], o_s[6], o_s[7]
    blending, pts_ref, xyz_prime, rgb_d, sigma_d, z_d, dist_d = o_d[2], o_d[3], o_d[5], o_d[6], o_d[7], o_d[8], o_d[9]
    delta_xyz = xyz_prime - xyz
    outs = R.raw2outputs(rgb_s, sigma_s, rgb_d, sigma_d, dist_d, blending, z_d, rays, ray_type=ray_type)
    weights_s, weights_d = outs[7], outs[11]
    sf_f, sf_b = dy.get_forward_backward_scene_flow(pts_ref, ts)
    pts_f = pts_ref + sf_f
    pts_b = pts_ref + sf_b
    n = weights_d.shape[0]
    tile = lambda p: torch.tile(p[None], (n, 1, 1))
    flow_f, _ = R.induce_flow(H, W, focal, tile(pose_f), weights_d, pts_f, grid2d, rays, ray_type=ray_type)
    flow_b, _ = R.induce_flow(H, W, focal, tile(pose_b), weights_d, pts_b, grid2d, rays, ray_type=ray_type)
    flow_s_f, _ = R.induce_flow(H, W, focal, tile(pose_f), weights_s, pts_ref_s, grid2d, rays, ray_type=ray_type)
    flow_s_b, _ = R.induce_flow(H, W, focal, tile(pose_b), weights_s, pts_ref_s, grid2d, rays, ray_type=ray_type)
    delta_sum = torch.sum(weights_d[..., None] * delta_xyz, 1)
    return dict(flow_f=flow_f, flow_b=flow_b, flow_s_f=flow_s_f, flow_s_b=flow_s_b, delta_xyz=delta_sum,
                acc_d=weights_d.sum(-1), rgb=outs[0], depth=outs[1])


def frame_rays(RU, c2w, focal, ray_type):
    d = RU.get_ray_directions_blender(H, W, [focal, focal])
    o, d = RU.get_rays(d, c2w)
    if ray_type == "ndc":
        o, d = RU.ndc_rays_blender(H, W, focal, 1.0, o, d)
    return torch.cat([o, d], 1).reshape(-1, 6)


def gen(name, mods, ray_type, act, static_head, grid, seed, density_shift):
    TS, TD, R, RU, CAM = mods
    import flow_viz
    aabb = torch.tensor([[-1.5, -1.67, -1.0], [1.5, 1.67, 1.0]]) if ray_type == "ndc" else \
        torch.tensor([[-2.0, -2.0, -2.0], [2.0, 2.0, 2.0]])
    st, dy = MG.build_fields(TS, TD, aabb, grid, act, static_head, density_shift, seed)
    if ray_type == "contract":
        st.near_far = [0.0, 256.0]
        dy.near_far = [0.0, 256.0]
    g = torch.Generator().manual_seed(seed + 1)
    focal = max(H, W) / 2.0 * 1.7320508
    p9 = torch.zeros(4, 9)    # (four rows: camera.pose_to_mtx's dim-less torch.cross takes a batch of three for the axis)
    p9[:, 0] = 1
    p9[:, 4] = 1
    p9 = p9 + 0.04 * torch.randn(4, 9, generator=g)
    poses = CAM.pose_to_mtx(p9).detach()       # own, next, previous frame
    rays = frame_rays(RU, poses[0], focal, ray_type).detach()
    ts = torch.full((H * W,), 2.0 * 5 / (T - 1) - 1.0)
    ii, jj = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32), indexing="xy")
    grid2d = torch.from_numpy(np.stack([ii, jj], -1)).view(-1, 2)
    ftn = torch.tensor(focal)

    def run():
        with torch.no_grad():
            return chain(R, st, dy, rays, ts, grid2d, ftn, poses[1], poses[2], ray_type)

    with torch.no_grad():   # conditioning (see the module docstring)
        for _ in range(200):
            out = run()
            if float((out["acc_d"] > 0.1).float().mean()) >= 0.5:
                break
            dy.density_layer2.bias += DENSITY_BIAS_STEP
        for _ in range(40):
            out = run()
            gap = min(float((out["flow_f"] - out["flow_s_f"]).abs().median()), float((out["flow_b"] - out["flow_s_b"]).abs().median()))
            if gap >= 1.0:
                break
            dy.scene_flow_mlp[6].weight *= SCENE_FLOW_SCALE_STEP
            dy.scene_flow_mlp[6].bias *= SCENE_FLOW_SCALE_STEP
    out = run()

    # the same chain in fp64 on the same weights
    torch.set_default_dtype(torch.float64)
    try:
        st64, dy64 = MG.build_fields(TS, TD, aabb.double(), grid, act, static_head, density_shift, seed)
        st64.near_far, dy64.near_far = st.near_far, dy.near_far
        st64.load_state_dict({k: v.double() for k, v in st.state_dict().items()})
        dy64.load_state_dict({k: v.double() for k, v in dy.state_dict().items()})
        st64, dy64 = st64.double(), dy64.double()
        with torch.no_grad():
            out64 = chain(R, st64, dy64, rays.double(), ts.double(), grid2d.double(), ftn.double(), poses[1].double(),
                          poses[2].double(), ray_type)
    finally:
        torch.set_default_dtype(torch.float32)
    spread = {k: float((out[k].double() - out64[k]).abs().max() / out64[k].abs().max()) for k in MAPS}

    stats = dict(
        gap_f=float((out["flow_f"] - out["flow_s_f"]).abs().median()),
        gap_b=float((out["flow_b"] - out["flow_s_b"]).abs().median()),
        delta_max=float(out["delta_xyz"].abs().max()),
        acc_frac=float((out["acc_d"] > 0.1).float().mean()),
        fp64_spread=max(spread.values()))
    print(name, {k: f"{v:.3g}" for k, v in stats.items()}, {k: f"{v:.1e}" for k, v in spread.items()})
    check(stats)

    res = {"meta.ray_type": np.array(ray_type), "meta.act": np.array(act), "meta.static_head": np.array(static_head),
           "meta.grid": np.array(grid), "meta.density_shift": np.array(density_shift, dtype=np.float32),
           "meta.near_far": np.array(dy.near_far, dtype=np.float32), "meta.H": np.array(H), "meta.W": np.array(W),
           "meta.S": np.array(S), "aabb": aabb.numpy(), "rays": rays.numpy(), "ts": ts.numpy(),
           "focal": np.array(focal, dtype=np.float32), "c2w": poses[0].numpy(), "c2w_f": poses[1].numpy(),
           "c2w_b": poses[2].numpy()}
    for k in MAPS + ("rgb", "depth", "acc_d"):
        res["out." + k] = out[k].numpy()
    res["stat.fp64_spread"] = np.array(stats["fp64_spread"])
    for k in MAPS[:4]:   # flow_to_image modifies its argument in place (inf -> 0): it gets a copy, the input is stored
        flow = out[k].view(H, W, 2).numpy().copy()
        res["viz." + k] = flow_viz.flow_to_image(flow.copy())
    # a picture of a flow with out-of-range radii is the same code path; one with inf / NaN entries is not:
    odd = out["flow_f"].view(H, W, 2).numpy().copy()
    odd[0, 0, 0] = np.inf
    odd[1, 2, 1] = -np.inf
    res["viz_inf.flow"] = odd.copy()
    res["viz_inf.image"] = flow_viz.flow_to_image(odd.copy())
    odd[3, 3, 0] = np.nan
    res["viz_nan.flow"] = odd.copy()
    with np.errstate(invalid="ignore"):
        res["viz_nan.image"] = flow_viz.flow_to_image(odd.copy())
    res["viz_zero.image"] = flow_viz.flow_to_image(np.zeros((H, W, 2), np.float32))
    MG.to_np(st.state_dict(), "s.", res)
    MG.to_np(dy.state_dict(), "d.", res)
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **res)
    print(f"{name}: {os.path.getsize(path) / 1024:.0f} KiB")


def check(stats):
    """what makes the fixture worth having (also asserted on the stored file by tests/test_motion_cpu.py)"""
    assert stats["gap_f"] >= 1.0 and stats["gap_b"] >= 1.0, stats
    assert stats["delta_max"] > 1e-3, stats
    assert stats["acc_frac"] >= 0.5, stats
    assert stats["fp64_spread"] <= 2e-5, stats


if __name__ == "__main__":
    mods = MG.import_reference()
    gen("motion_ndc", mods, "ndc", "softplus", "MLP_Fea", [14, 15, 9], 20260301, -1.0)
    gen("motion_contract", mods, "contract", "softplus", "MLP_Fea_TimeEmbedding", [10, 10, 10], 20260302, -1.0)
