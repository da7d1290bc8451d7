"""Float64 reference of the per-point field evaluation (csrc/rdrf_point.hip, fields.TensorBase.query_points): what
TensorBase.forward gives ONE sample with ray_valid = 1 at a position, a time and a view direction -- no ray, no transmittance,
no weight threshold.  Composed from the oracle's pieces (normalize_coord, vm_features, _planes, positional_encoding) the way
tests/_gpu_util.py::kink_free_rays composes them; every tensor is taken to float64 first.  tests/test_point_query_cpu.py holds
it to the reference-generated goldens on their own sample points."""
import torch
import torch.nn.functional as F

from oracle import rodynrf_oracle as O


def _f64(sd):
    return {k: v.detach().double() for k, v in sd.items()}


def _lin(x, sd, name):
    return F.linear(x, sd[name + ".weight"], sd.get(name + ".bias"))


def _act(f, cfg):
    return F.softplus(f + cfg["density_shift"]) if cfg["act"] == "softplus" else F.relu(f)


def point_reference(sd, cfg, xyz, t, viewdirs, dynamic):
    """sd / cfg: a golden case's state dict and config (tests/_util.load_case).  xyz [M,3] un-normalised, t [M] (dynamic
    field; ignored by the static one), viewdirs [M,3] used as given.  -> dict of float64 tensors: sigma [M], rgb [M,3] and,
    for the dynamic field, blending [M] and xyz_prime [M,3]."""
    pe = O.positional_encoding
    with torch.no_grad():
        sd = _f64(sd)
        aabb = torch.as_tensor(cfg["aabb"]).double()
        xyz, vd = torch.as_tensor(xyz).double().reshape(-1, 3), torch.as_tensor(viewdirs).double().reshape(-1, 3)
        xn = O.normalize_coord(xyz, aabb)
        if not dynamic:
            sigma = _act(O.vm_features(*O._planes(sd, "density"), xn).sum(-1), cfg)
            af = F.linear(O.vm_features(*O._planes(sd, "app"), xn), sd["basis_mat.weight"])
            if cfg["head"] == "MLP_Fea":
                x = F.relu(_lin(torch.cat([af, vd, pe(af, 2)], -1), sd, "renderModule.mlp.0"))
                x = F.relu(_lin(x, sd, "renderModule.mlp.2"))
                rgb = torch.sigmoid(_lin(x, sd, "renderModule.mlp.4"))
            else:
                x = F.relu(_lin(torch.cat([af, pe(af, 2)], -1), sd, "renderModule.mlp.0"))
                x = F.relu(_lin(x, sd, "renderModule.mlp.2"))
                rgb = torch.sigmoid(_lin(torch.cat([x, vd], -1), sd, "renderModule.mlp_view.0"))
            return {"sigma": sigma, "rgb": rgb}
        tt = torch.as_tensor(t).double().reshape(-1, 1)
        tout = _lin(F.relu(_lin(torch.cat([tt, pe(tt, 8)], -1), sd, "layer1")), sd, "layer2")
        h = F.relu(_lin(torch.cat([xn, pe(xn, 10), tout], -1), sd, "layer3"))
        d = _lin(F.relu(_lin(h, sd, "layer4")), sd, "layer5")
        xw = O.normalize_coord(O.unnormalize_coord(xn, aabb) + d, aabb)
        tail = [xn, pe(xn, 10), tt, pe(tt, 8)]
        raw = {}
        for prefix in ("density", "blending"):
            feats = O.vm_features(*O._planes(sd, prefix), xw, (1, 2, 4))
            raw[prefix] = _lin(F.relu(_lin(torch.cat([feats] + tail, -1), sd, prefix + "_layer1")), sd, prefix + "_layer2")[..., 0]
        af = F.linear(O.vm_features(*O._planes(sd, "app"), xw, (1, 2, 4)), sd["basis_mat.weight"])
        x = F.relu(_lin(torch.cat([af] + tail, -1), sd, "renderModule.mlp.0"))
        x = F.relu(_lin(x, sd, "renderModule.mlp.2"))
        rgb = torch.sigmoid(_lin(torch.cat([x, vd], -1), sd, "renderModule.mlp_view.0"))
        return {"sigma": _act(raw["density"], cfg), "blending": torch.sigmoid(raw["blending"]), "rgb": rgb, "xyz_prime": xyz + d}


def golden_points(g, rt):
    """the sample points of a golden case as a point batch: (xyz [N*S,3], t [N*S], viewdirs [N*S,3] formed as ray_norm forms
    them -- normalised for ndc / contract rays), float32"""
    rays, ts, xyz = torch.from_numpy(g["rays"]), torch.from_numpy(g["ts"]), torch.from_numpy(g["xyz"])
    N, S = xyz.shape[:2]
    _, vd = O._dists_viewdirs(rays, torch.from_numpy(g["z"]), rt)
    return xyz.reshape(-1, 3), ts[:, None].expand(N, S).reshape(-1), vd[:, None, :].expand(N, S, 3).reshape(-1, 3)


def ray_norm_viewdirs(rays):
    """The bits csrc/rdrf_kernels.hpp ray_norm hands the appearance kernels for ndc / contract rays [N,6] -> [N,3] float32.
    The compiler contracts vx vx + vy vy + vz vz into fma(vx, vx, vy vy) + vz vz there (one rounding for the first two
    terms), the square root and the three quotients are correctly rounded; the fma is formed exactly in rationals here."""
    from fractions import Fraction
    import numpy as np
    f = np.float32
    d = np.ascontiguousarray(torch.as_tensor(rays)[:, 3:6].cpu().numpy(), dtype=np.float32)
    out = np.empty_like(d)
    for i, (vx, vy, vz) in enumerate(d):
        yy = f(vy * vy)
        s = f(float(Fraction(float(vx)) * Fraction(float(vx)) + Fraction(float(yy))))
        nrm = np.sqrt(f(s + f(vz * vz)), dtype=np.float32)
        out[i] = d[i] / nrm
    return torch.from_numpy(out)
