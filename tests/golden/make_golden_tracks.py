"""Fixture of the point tracks: tests/golden/tracks.npz.

Runs only where the reference is available (it is imported through make_golden.import_reference; nothing of it is
copied).  One seeded dynamic field (the reference's TensorVMSplit_TimeEmbedding; its weights do not depend on the box, so
the ndc and the contract case share them -- asserted below) and 70 seed points per ray type.  Stored:

  * the field's weights (the "d." layout tests/_util.load_case reads) and both boxes
  * the reference's get_forward_backward_scene_flow_point_single outputs on the seeds
  * a chain of 5 forward and 3 backward steps per ray type, made by looping the reference's OWN calls: _point_single for the
    step, torch.clamp(., -2 + 1e-6, 2 - 1e-6) for contract (train.py:1377-1378), t +- 2 / (T - 1) in fp32, and for ndc
    render_single_3d_point of every slot into that slot's camera

The scene-flow MLP's last layer is scaled until a step moves a point by >= 0.02 (median), so that a chain is not a
constant; some ndc seeds sit at z near 1 (NDC2world's clamp) and some contract seeds at 1.99 (the step clamp fires): both
asserted.

    python tests/golden/make_golden_tracks.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402

M, T, N_FWD, N_BWD, H, W = 70, 12, 5, 3, 12, 16
GRID = [9, 10, 7]
SEED = 20260611
SCENE_FLOW_SCALE_STEP = 2.0
LO, HI = -2.0 + 1e-6, 2.0 - 1e-6


def chain(R, dy, p0, t0, ray_type, cams, focal):
    """slots 0 .. N_BWD + N_FWD (slot N_BWD = the seed) by the reference's own calls"""
    K = N_BWD + 1 + N_FWD
    dt = 2.0 / (T - 1)
    pts = [None] * K
    pts[N_BWD] = p0
    for d, n in ((0, N_FWD), (1, N_BWD)):
        p, t = p0, t0
        for k in range(1, n + 1):
            nxt = dy.get_forward_backward_scene_flow_point_single(p, t)[d]
            if ray_type == "contract":
                nxt = torch.clamp(nxt, min=LO, max=HI)
            p = nxt
            t = t + dt if d == 0 else t - dt
            pts[N_BWD + k if d == 0 else N_BWD - k] = p
    out = {"pts": torch.stack(pts, 1)}
    if ray_type == "ndc":
        proj = [R.render_single_3d_point(H, W, focal, torch.tile(cams[k][None], (M, 1, 1)), pts[k]) for k in range(K)]
        out["pix"] = torch.stack([a for a, _ in proj], 1)
        out["disp"] = torch.stack([b[:, 0] for _, b in proj], 1)
    return out


def main():
    TS, TD, R, RU, CAM = MG.import_reference()
    boxes = {"ndc": torch.tensor([[-1.5, -1.67, -1.0], [1.5, 1.67, 1.0]]),
             "contract": torch.tensor([[-2.0, -2.0, -2.0], [2.0, 2.0, 2.0]])}
    fields = {rt: MG.build_fields(TS, TD, boxes[rt], GRID, "softplus", "MLP_Fea", -1.0, SEED)[1] for rt in boxes}
    sd = {rt: {k: v for k, v in fields[rt].state_dict().items()} for rt in boxes}
    shared = [k for k in sd["ndc"] if torch.equal(sd["ndc"][k], sd["contract"][k])]
    assert all(k in shared for k in sd["ndc"] if "scene_flow_mlp" in k), "the scene-flow weights depend on the box"
    g = torch.Generator().manual_seed(SEED + 1)
    frames = torch.randint(N_BWD, T - N_FWD, (M,), generator=g)
    t0 = frames.float() * 2 / (T - 1) - 1
    seeds = {}
    lo, hi = boxes["ndc"]
    p = lo + (hi - lo) * torch.rand(M, 3, generator=g)
    p[:8, 2] = torch.tensor([1.0, 0.9999999, 0.999999, 0.99999, 1.0 + 1e-6, 0.9999995, 0.999, 1.01])   # NDC2world's clamp
    seeds["ndc"] = p
    p = -1.9 + 3.8 * torch.rand(M, 3, generator=g)
    p[:6] = 1.99 * torch.sign(p[:6])     # the step clamp
    p[6:10, 0] = -1.99
    seeds["contract"] = p
    p9 = torch.zeros(N_BWD + 1 + N_FWD, 9)
    p9[:, 0] = 1
    p9[:, 4] = 1
    p9 = p9 + 0.04 * torch.randn(p9.shape, generator=g)
    cams = CAM.pose_to_mtx(p9).detach()
    focal = torch.tensor(max(H, W) / 2.0 * 1.7320508)

    with torch.no_grad():
        for _ in range(40):   # conditioning: a step moves a point
            sf = fields["ndc"].get_forward_backward_scene_flow_point_single(seeds["ndc"], t0)[2]
            if float(sf.abs().median()) >= 0.02:
                break
            for dy in fields.values():
                dy.scene_flow_mlp[6].weight *= SCENE_FLOW_SCALE_STEP
                dy.scene_flow_mlp[6].bias *= SCENE_FLOW_SCALE_STEP
        res = {"meta.M": np.array(M), "meta.T": np.array(T), "meta.n_fwd": np.array(N_FWD), "meta.n_bwd": np.array(N_BWD),
               "meta.H": np.array(H), "meta.W": np.array(W), "meta.grid": np.array(GRID), "meta.act": np.array("softplus"),
               "meta.density_shift": np.array(-1.0, dtype=np.float32), "t0": t0.numpy(), "cams": cams.numpy(),
               "focal": focal.numpy()}
        for rt, dy in fields.items():
            single = dy.get_forward_backward_scene_flow_point_single(seeds[rt], t0)
            for name, v in zip(("pts_f", "pts_b", "sf_f", "sf_b"), single):
                res[f"{rt}.single.{name}"] = v.numpy()
            ch = chain(R, dy, seeds[rt], t0, rt, cams, focal)
            for k, v in ch.items():
                assert torch.isfinite(v).all(), (rt, k)
                res[f"{rt}.chain.{k}"] = v.numpy()
            res[f"{rt}.aabb"] = boxes[rt].numpy()
            res[f"{rt}.p0"] = seeds[rt].numpy()
            step = float((ch["pts"][:, 1:] - ch["pts"][:, :-1]).abs().median())
            print(rt, f"median step {step:.3g}", f"max |pts| {float(ch['pts'].abs().max()):.4g}")
            assert step >= 0.005, step
        c = res["contract.chain.pts"]
        assert (np.abs(c[:, np.arange(c.shape[1]) != N_BWD]) == np.float32(HI)).any(), "the clamp does not fire"
        assert (res["ndc.p0"][:, 2] >= 1 - 1e-6).sum() >= 3
    MG.to_np(fields["ndc"].state_dict(), "d.", res)
    path = os.path.join(HERE, "tracks.npz")
    np.savez_compressed(path, **res)
    print(f"tracks: {os.path.getsize(path) / 1024:.0f} KiB")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
