"""Host-side mirror of the reference field objects for the ray-batch hot path.

``TensorVMSplit`` / ``TensorVMSplit_TimeEmbedding`` keep the reference's constructor kwargs,
attribute names, ``state_dict`` keys/shapes, ``get_optparam_groups`` and the
``forward(rays_chunk, ts_chunk, timeembeddings_chunk, xyz_sampled, z_vals, ray_valid, ...)``
10-tuple (/root/reference/models/tensorBase.py:281-339, 704-850; models/tensoRF.py:11-61,
277-376), but every per-sample computation runs in the HIP kernels behind the C ABI
(include/rodynrf.h).  The nn.Linear / nn.Sequential objects here are parameter containers only.

VM factors are stored channel-last: a plane parameter has the reference's logical shape
(1,C,H,W) with strides of an [H][W][C] array, so state_dicts interchange with the reference while
one bilinear tap of 4 components is a single 16-byte load on the GPU.
"""
import collections
import ctypes as C

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib as L
# the struct builders live in _params; tests and tools reach them as fields._vm_struct, fields._attach_packed, ...
from ._params import _attach_packed, _cfg_struct, _dynamic_struct, _static_struct, _vm_struct, field_structs  # noqa: F401
from .regularizers import _tensor4, dense_l1, tv_family, vector_diffs

MAT_MODE = [[0, 1], [0, 2], [1, 2]]
# packed weight images (_params._attach_packed): handed to the entry points instead of a re-pack per call; 0 switches them off
PACK_CACHE = os.environ.get("RDRF_PACK_CACHE", "1") == "1"
VEC_MODE = [2, 1, 0]
# the 10-tuple both fields' forward returns, in the reference's order (models/tensorBase.py:814-850): per-sample tensors
# [N,S(,3)]; the static field has no blending / xyz_prime (None), rgb is None under forward(rgb=False)
FieldOut = collections.namedtuple("FieldOut", ("unused0", "unused1", "blending", "xyz_sampled", "weight", "xyz_prime", "rgb",
                                               "sigma", "z_vals", "dists"))


# --------------------------------------------------------------------------------------------
# parameter containers (same attribute / key structure as models/tensorBase.py:81-183)
# --------------------------------------------------------------------------------------------
class _Head(nn.Module):
    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError("the RGB head is fused into the HIP appearance kernel; call the field")


class MLPRender_Fea(_Head):
    def __init__(self, inChanel, viewpe=6, feape=6, featureC=128):
        super().__init__()
        self.in_mlpC = 2 * viewpe * 3 + 2 * feape * inChanel + 3 + inChanel
        self.viewpe, self.feape = viewpe, feape
        self.mlp = nn.Sequential(nn.Linear(self.in_mlpC, featureC), nn.ReLU(inplace=True),
                                 nn.Linear(featureC, featureC), nn.ReLU(inplace=True),
                                 nn.Linear(featureC, 3))
        nn.init.constant_(self.mlp[-1].bias, 0)


class MLPRender_Fea_TimeEmbedding(_Head):
    def __init__(self, inChanel, viewpe=6, feape=6, featureC=128):
        super().__init__()
        self.in_mlpC = 2 * feape * inChanel + inChanel
        self.in_view = 2 * viewpe * 3 + 3
        self.viewpe, self.feape = viewpe, feape
        layer1 = nn.Linear(self.in_mlpC, featureC)
        layer2 = nn.Linear(featureC, featureC)
        layer3 = nn.Linear(featureC + self.in_view, 3)
        self.mlp = nn.Sequential(layer1, nn.ReLU(inplace=True), layer2, nn.ReLU(inplace=True))
        self.mlp_view = nn.Sequential(layer3)
        nn.init.constant_(self.mlp_view[-1].bias, 0)


class MLPRender_Fea_late_view(_Head):
    def __init__(self, inChanel, viewpe=6, feape=6, featureC=128):
        super().__init__()
        self.in_mlpC = 2 * feape * inChanel + inChanel + 2 * 10 * 3 + 3 + 2 * 8 * 1 + 1
        self.in_view = 2 * viewpe * 3 + 3
        self.viewpe, self.feape = viewpe, feape
        layer1 = nn.Linear(self.in_mlpC, featureC)
        layer2 = nn.Linear(featureC, featureC)
        layer3 = nn.Linear(featureC + self.in_view, 3)
        self.mlp = nn.Sequential(layer1, nn.ReLU(inplace=True), layer2, nn.ReLU(inplace=True))
        self.mlp_view = nn.Sequential(layer3)
        nn.init.constant_(self.mlp_view[-1].bias, 0)


# storage order of the XZ / YZ planes: False = [z][x|y][C] (x fastest: the two bilinear columns of a
# tap are 16-32 bytes apart and the scatter's column-split atomics merge into one L2 request each);
# True = [x|y][z][C].  The kernels take explicit strides, either works.
Z_FAST = os.environ.get("RDRF_Z_FAST", "0") == "1"


def channel_last_(t, h_fast=False):
    """Re-stride a (1,C,H,W) tensor with the component axis contiguous (values preserved):
    [H][W][C] by default, [W][H][C] when `h_fast` (used for the XZ / YZ planes, whose H axis is z:
    consecutive samples of a forward-facing ray then read / update adjacent texels)."""
    _, c, h, w = t.shape
    strides = (c * h * w, 1, c, h * c) if h_fast else (c * h * w, 1, w * c, c)
    out = torch.empty_strided(t.shape, strides, dtype=t.dtype, device=t.device)
    out.copy_(t)
    return out


def _is_channel_last(t):
    return t.stride(1) == 1 or t.numel() == 0


# --------------------------------------------------------------------------------------------
# autograd bridges
# --------------------------------------------------------------------------------------------
# Saved-byte accounting: per kind of call (0 static field, 1 dynamic field, 2 scene flow, "feat0" / "feat1" the
# per-point entry points) the number of forwards that saved "full" rows, "no_app" rows (RDRF_SAVE_NO_APP) or "none", and the
# bytes allocated for them -- what the trainer's tests read to see which forward saved what.
SAVE_STATS = collections.Counter()


def _call_modes(rgb):
    """-> (rgb mode, grad mode): what the field modules hand to their autograd Function next to the ray type.  rgb mode:
    forward()'s `rgb`, True, False or "value".  Grad mode: rows are saved only where a backward can read them.  Under
    torch.no_grad() none can exist, yet ctx.needs_input_grad still reports True for parameters there -- and inside
    Function.forward grad mode is always off -- so the modules capture the CALLER's mode here and hand it in."""
    rgb = rgb if isinstance(rgb, str) else bool(rgb)
    if rgb not in (True, False, "value"):
        raise ValueError(f"forward(..., rgb=...) takes True, False or 'value', not {rgb!r}")
    return rgb, torch.is_grad_enabled()


def _saved(ctx, key, nbytes, dev, grad_mode, rows="full"):
    """training mode: a per-call buffer the forward fills with the activations its backward needs (inference -- the caller
    runs under no_grad, or no input requires grad -- keeps nothing).  grad_mode None = the mode right here."""
    if not (torch.is_grad_enabled() if grad_mode is None else grad_mode) or not any(ctx.needs_input_grad):
        SAVE_STATS[(key, "none")] += 1
        return None, 0
    nbytes = int(nbytes())
    SAVE_STATS[(key, rows)] += 1
    SAVE_STATS[(key, "bytes")] += nbytes
    return torch.empty(nbytes, dtype=torch.uint8, device=dev), nbytes


def _alloc_saved(ctx, kind, N, S, dev, grad_mode=None, flags=0):
    """the saved buffer of a field / scene-flow forward (see _saved).  flags: RDRF_SAVE_* of rdrf_saved_bytes_ex
    (L.SAVE_NO_APP: the colours are values only, no appearance rows)."""
    return _saved(ctx, kind, lambda: L.lib.rdrf_saved_bytes_ex(kind, N, S, flags), dev, grad_mode,
                  "no_app" if flags & L.SAVE_NO_APP else "full")


def _feat_saved(ctx, dynamic, M, dev, grad_mode=None):
    """the saved buffer of a per-point forward (see _saved)"""
    return _saved(ctx, "feat%d" % int(dynamic), lambda: L.lib.rdrf_features_saved_bytes(int(dynamic), M), dev, grad_mode)


def _input(t):
    """a tensor as the entry points read it: contiguous fp32, masks as uint8"""
    if t.dtype in (torch.bool, torch.uint8):
        t = t.contiguous()
        return t.view(torch.uint8) if t.dtype == torch.bool else t
    return L.f32c(t)


def _begin_forward(ctx, field, params, ray_type, inputs, dims, saved, ws_bytes):
    """What the five forwards share.  Checks and converts `inputs`, takes the saved buffer (`saved(dev)`: _alloc_saved or
    _feat_saved of this call) and the workspace (`ws_bytes(saved is not None)` bytes), builds the structs and stashes in ctx
    what the backward reads.  Returns (head, tail, saved buffer): every forward entry point is called as
    fn(*head, *dims, outputs..., *tail) with head = P, cfg, the inputs and tail = saved, saved_bytes, ws, ws_bytes, stream."""
    ctx.set_materialize_grads(False)   # unused outputs arrive as None: their branch is skipped
    L.require_device(*inputs)
    inputs = [_input(t) for t in inputs]
    dev = inputs[0].device
    buf, sbytes = saved(dev)
    ws = L.workspace(dev, ws_bytes(buf is not None))
    P, cfg = field_structs(field, params, ray_type)
    ctx.field, ctx.ray_type, ctx.dims, ctx.saved = field, ray_type, dims, buf
    ctx.save_for_backward(*inputs, *params)
    return ((C.byref(P), C.byref(cfg), *[L.ptr(t) for t in inputs]),
            (L.ptr(buf), sbytes, L.ptr(ws), ws.numel(), L.stream_of(inputs[0])), buf)


def _begin_backward(ctx, n_inputs, twice, cotangents, ws_bytes):
    """What the five backwards share once they know there is something to differentiate.  Refuses a second backward (with
    the message `twice`), binds the deterministic build's shadow, takes the gradient buffers (the field's flat buffer when
    fused_grad) and the workspace (`ws_bytes(*dims)` bytes) and builds the structs.  Returns (inputs, head, cot, G, tail,
    grads): every backward entry point is called as fn(*head, *dims, cotangents..., G, input gradients..., *tail) with `cot`
    the contiguous cotangents; `grads` goes through _end_backward into the return tuple."""
    tensors = ctx.saved_tensors
    inputs, params = tensors[:n_inputs], tensors[n_inputs:]
    if ctx.saved is None:
        raise L.RdrfError(twice)
    field = ctx.field
    field._det_bind()
    grads = field.fused_grads() if field.fused_grad else [torch.zeros_like(p) for p in params]
    G = (_dynamic_struct if field.DYNAMIC else _static_struct)(grads)
    P, cfg = field_structs(field, params, ctx.ray_type, True)
    ws = L.workspace(inputs[0].device, ws_bytes(*ctx.dims))
    return (inputs, (C.byref(P), C.byref(cfg), *[L.ptr(t) for t in inputs]), [None if g is None else L.f32c(g) for g in cotangents],
            C.byref(G), (L.ptr(ctx.saved), ctx.saved.numel(), L.ptr(ws), ws.numel(), L.stream_of(inputs[0])), grads)


def _end_backward(ctx, grads):
    """release the saved activations; the parameter gradients to return: None when fused (already accumulated into
    p.grad, views of the field's flat buffer)"""
    ctx.saved = None
    return [None] * len(grads) if ctx.field.fused_grad else grads


def _field_forward(ctx, kind, field, ray_type, rgb_mode, grad_mode, inputs, params):
    """the forward of _StaticFn / _DynamicFn up to the entry point -> (N, S, rgb, flags, head, tail).  rgb=False -- the
    colours are not wanted; rgb="value" -- computed, but no gradient will be asked for them: no appearance rows are saved.
    A call that saves nothing takes the smaller forward workspace."""
    N, S = inputs[3].shape
    flags = L.SAVE_NO_APP if rgb_mode == "value" else 0
    head, tail, _ = _begin_forward(
        ctx, field, params, ray_type, inputs, (N, S), lambda dev: _alloc_saved(ctx, kind, N, S, dev, grad_mode, flags),
        lambda saving: (L.lib.rdrf_workspace_bytes if saving else L.lib.rdrf_forward_workspace_bytes)(N, S))
    rgb = torch.empty(N, S, 3, device=inputs[3].device) if rgb_mode is not False else None
    if rgb_mode == "value":
        ctx.mark_non_differentiable(rgb)
    ctx.want_rgb = rgb_mode is True
    return N, S, rgb, flags, head, tail


def _field_backward(ctx, entry, what, twice, cotangents, g_rgb):
    """the backward of _StaticFn / _DynamicFn: they differ in the entry point and its cotangents, g_dists last"""
    if g_rgb is not None and not ctx.want_rgb:
        raise L.RdrfError("forward(..., rgb=False | 'value') saved no appearance rows: no gradient can flow through rgb")
    need = ctx.needs_input_grad   # field, ray_type, rgb_mode, grad_mode, rays, ts, xyz, z, valid, *params
    if all(g is None for g in cotangents[:-1]) and not (need[4] or need[7]):
        # only `dists` is consumed downstream (pass E of the trainer feeds the dynamic field's dists to the compositor): it
        # depends on z_vals and |d| alone, no parameter (and here neither rays nor z_vals want a gradient) -- nothing to
        # differentiate, exactly as in the reference where dists has no parameter ancestry
        ctx.saved = None
        return (None,) * len(need)
    (rays, _, xyz, z, _), head, cot, G, tail, grads = _begin_backward(ctx, 5, twice, cotangents, L.lib.rdrf_workspace_bytes)
    g_rays, g_xyz, g_z = L.zeros_like_many([rays, xyz, z], [need[4], need[6], need[7]])
    L.check(entry(*head, *ctx.dims, *map(L.ptr, cot), G, L.ptr(g_xyz), L.ptr(g_z), L.ptr(g_rays), *tail), what)
    return (None, None, None, None, g_rays, None, g_xyz, g_z, None, *_end_backward(ctx, grads))


class _StaticFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, field, ray_type, rgb_mode, grad_mode, rays, ts, xyz, z, valid, *params):
        N, S, rgb, flags, head, tail = _field_forward(ctx, 0, field, ray_type, rgb_mode, grad_mode, (rays, ts, xyz, z, valid), params)
        sigma, weight, dists = (torch.empty(N, S, device=z.device) for _ in range(3))
        L.check(L.lib.rdrf_static_fwd_ex(*head, N, S, L.ptr(rgb), L.ptr(sigma), L.ptr(weight), L.ptr(dists), *tail, flags),
                "rdrf_static_fwd")
        return rgb, sigma, weight, dists

    @staticmethod
    def backward(ctx, g_rgb, g_sigma, g_weight, g_dists):
        return _field_backward(ctx, L.lib.rdrf_static_bwd, "rdrf_static_bwd",
                               "TensorVMSplit.forward: backward called twice (the saved activations are released "
                               "after the first backward; retain_graph is not supported)",
                               (g_rgb, g_sigma, g_weight, g_dists), g_rgb)


class _DynamicFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, field, ray_type, rgb_mode, grad_mode, rays, ts, xyz, z, valid, *params):
        N, S, rgb, flags, head, tail = _field_forward(ctx, 1, field, ray_type, rgb_mode, grad_mode, (rays, ts, xyz, z, valid), params)
        xyz_prime = torch.empty(N, S, 3, device=z.device)
        sigma, weight, dists, blending = (torch.empty(N, S, device=z.device) for _ in range(4))
        L.check(L.lib.rdrf_dynamic_fwd_ex(*head, N, S, L.ptr(blending), L.ptr(weight), L.ptr(xyz_prime), L.ptr(rgb), L.ptr(sigma),
                                          L.ptr(dists), *tail, flags), "rdrf_dynamic_fwd")
        return blending, weight, xyz_prime, rgb, sigma, dists

    @staticmethod
    def backward(ctx, g_blending, g_weight, g_xyz_prime, g_rgb, g_sigma, g_dists):
        return _field_backward(ctx, L.lib.rdrf_dynamic_bwd, "rdrf_dynamic_bwd",
                               "TensorVMSplit_TimeEmbedding.forward: backward called twice (the saved activations "
                               "are released after the first backward; retain_graph is not supported)",
                               (g_blending, g_weight, g_xyz_prime, g_rgb, g_sigma, g_dists), g_rgb)


class _SceneFlowFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, field, grad_mode, pts, ts, *params):
        N, S, _ = pts.shape
        head, tail, _ = _begin_forward(ctx, field, params, "ndc", (pts, ts), (N, S),
                                       lambda dev: _alloc_saved(ctx, 2, N, S, dev, grad_mode),
                                       lambda saving: L.lib.rdrf_workspace_bytes(N, S))
        sf_f = torch.empty(N, S, 3, device=pts.device)
        sf_b = torch.empty(N, S, 3, device=pts.device)
        L.check(L.lib.rdrf_scene_flow_fwd(*head, N, S, L.ptr(sf_f), L.ptr(sf_b), *tail), "rdrf_scene_flow_fwd")
        return sf_f, sf_b

    @staticmethod
    def backward(ctx, g_f, g_b):
        (pts, _), head, cot, G, tail, grads = _begin_backward(
            ctx, 2, "get_forward_backward_scene_flow: backward called twice (retain_graph is not supported)", (g_f, g_b),
            L.lib.rdrf_workspace_bytes)
        g_pts = torch.zeros_like(pts) if ctx.needs_input_grad[2] else None
        L.check(L.lib.rdrf_scene_flow_bwd(*head, *ctx.dims, *map(L.ptr, cot), G, L.ptr(g_pts), *tail), "rdrf_scene_flow_bwd")
        return (None, None, g_pts, None, *_end_backward(ctx, grads))


# --------------------------------------------------------------------------------------------
# compute_* / warp_coordinate: the per-point building blocks (rdrf_*_features_fwd/bwd)
# --------------------------------------------------------------------------------------------
_FEAT_TWICE = "compute_*: backward called twice (the saved activations were released)"


class _StaticFeatFn(torch.autograd.Function):
    """(density feature [M], appearance feature [M,27]) of the static field at normalised points"""

    @staticmethod
    def forward(ctx, field, grad_mode, want_density, want_app, xn, *params):
        M, dev = xn.shape[0], xn.device
        head, tail, _ = _begin_forward(ctx, field, params, "ndc", (xn,), (M,), lambda dev: _feat_saved(ctx, 0, M, dev, grad_mode),
                                       lambda saving: L.lib.rdrf_features_workspace_bytes(M))
        dens = torch.empty(M, device=dev) if want_density else None
        app = torch.empty(M, 27, device=dev) if want_app else None
        L.check(L.lib.rdrf_static_features_fwd(*head, M, L.ptr(dens), L.ptr(app), *tail), "rdrf_static_features_fwd")
        return dens, app

    @staticmethod
    def backward(ctx, g_dens, g_app):
        if g_dens is None and g_app is None:
            return (None,) * len(ctx.needs_input_grad)
        (xn,), head, cot, G, tail, grads = _begin_backward(ctx, 1, _FEAT_TWICE, (g_dens, g_app),
                                                           L.lib.rdrf_features_bwd_workspace_bytes)
        g_xn = torch.zeros_like(xn) if ctx.needs_input_grad[4] else None
        L.check(L.lib.rdrf_static_features_bwd(*head, *ctx.dims, *map(L.ptr, cot), G, L.ptr(g_xn), *tail), "rdrf_static_features_bwd")
        return (None, None, None, None, g_xn, *_end_backward(ctx, grads))


class _DynFeatFn(torch.autograd.Function):
    """(density [M], blending [M], app [M,27], xyz_prime [M,3]) of the dynamic field at M points with
    per-point times; `x` normalised (compute_*) or un-normalised (warp_coordinate)"""

    @staticmethod
    def forward(ctx, field, grad_mode, want, x_is_normalized, x, t, *params):
        M, dev = x.shape[0], x.device
        head, tail, _ = _begin_forward(ctx, field, params, "ndc", (x, t), (M, int(x_is_normalized)),
                                       lambda dev: _feat_saved(ctx, 1, M, dev, grad_mode),
                                       lambda saving: L.lib.rdrf_features_workspace_bytes(M))
        dens = torch.empty(M, device=dev) if "density" in want else None
        blend = torch.empty(M, device=dev) if "blending" in want else None
        app = torch.empty(M, 27, device=dev) if "app" in want else None
        xp = torch.empty(M, 3, device=dev) if "warp" in want else None
        L.check(L.lib.rdrf_dynamic_features_fwd(*head, *ctx.dims, L.ptr(dens), L.ptr(blend), L.ptr(app), L.ptr(xp), *tail),
                "rdrf_dynamic_features_fwd")
        return dens, blend, app, xp

    @staticmethod
    def backward(ctx, g_dens, g_blend, g_app, g_xp):
        if all(g is None for g in (g_dens, g_blend, g_app, g_xp)):
            return (None,) * len(ctx.needs_input_grad)
        (x, _), head, cot, G, tail, grads = _begin_backward(ctx, 2, _FEAT_TWICE, (g_dens, g_blend, g_app, g_xp),
                                                            lambda M, norm: L.lib.rdrf_features_bwd_workspace_bytes(M))
        g_x = torch.zeros_like(x) if ctx.needs_input_grad[4] else None
        L.check(L.lib.rdrf_dynamic_features_bwd(*head, *ctx.dims, *map(L.ptr, cot), G, L.ptr(g_x), *tail), "rdrf_dynamic_features_bwd")
        return (None, None, None, None, g_x, None, *_end_backward(ctx, grads))


# --------------------------------------------------------------------------------------------
# TensorBase (models/tensorBase.py:281-559)
# --------------------------------------------------------------------------------------------
class TensorBase(nn.Module):
    def __init__(self, aabb, gridSize, tSize, device, density_n_comp=8, appearance_n_comp=24,
                 app_dim=27, shadingMode="MLP_PE", alphaMask=None, near_far=[2.0, 6.0],
                 density_shift=-10, alphaMask_thres=0.001, distance_scale=25,
                 rayMarch_weight_thres=0.0001, pos_pe=6, view_pe=6, fea_pe=6, featureC=128,
                 step_ratio=2.0, fea2denseAct="softplus"):
        super().__init__()
        self.density_n_comp = list(density_n_comp)
        self.app_n_comp = list(appearance_n_comp)
        self.app_dim = app_dim
        self.aabb = torch.as_tensor(aabb, dtype=torch.float32).to(device)
        self._aabb_host = [float(v) for v in self.aabb.detach().cpu().reshape(-1)]
        self.alphaMask = alphaMask
        self.device = device
        self.density_shift = density_shift
        self.alphaMask_thres = alphaMask_thres
        self.distance_scale = distance_scale
        self.rayMarch_weight_thres = rayMarch_weight_thres
        self.fea2denseAct = fea2denseAct
        self.near_far = near_far
        self.step_ratio = step_ratio
        self.tSizeFixed = tSize
        self.update_stepSize(gridSize, tSize)
        self.matMode = MAT_MODE
        self.vecMode = VEC_MODE
        self.comp_w = [1, 1, 1]
        if self.density_n_comp != [16, 4, 4] or self.app_n_comp != [48, 12, 12] or app_dim != 27 \
                or featureC != 128 or view_pe != 0:
            raise NotImplementedError(
                "the HIP kernels are built for the shipped configs: density comps [16,4,4], "
                "appearance comps [48,12,12], app_dim 27, featureC 128, view_pe 0")
        self.init_svd_volume(gridSize[0], device)
        self.shadingMode, self.pos_pe, self.view_pe, self.fea_pe, self.featureC = (
            shadingMode, pos_pe, view_pe, fea_pe, featureC)
        self.init_render_func(shadingMode, pos_pe, view_pe, fea_pe, featureC, device)

    # ---- construction ------------------------------------------------------------------
    def init_render_func(self, shadingMode, pos_pe, view_pe, fea_pe, featureC, device):
        if shadingMode == "MLP_Fea":
            self.renderModule = MLPRender_Fea(self.app_dim, view_pe, fea_pe, featureC).to(device)
        elif shadingMode == "MLP_Fea_TimeEmbedding":
            self.renderModule = MLPRender_Fea_TimeEmbedding(self.app_dim, view_pe, fea_pe,
                                                            featureC).to(device)
        elif shadingMode == "MLP_Fea_late_view":
            self.renderModule = MLPRender_Fea_late_view(self.app_dim, view_pe, fea_pe,
                                                        featureC).to(device)
        else:
            raise NotImplementedError(f"shadingMode {shadingMode} is not reachable from the shipped "
                                      "configs and is not built")

    def update_stepSize(self, gridSize, tSize):
        self.aabbSize = self.aabb[1] - self.aabb[0]
        self.invaabbSize = 2.0 / self.aabbSize
        self.gridSize = torch.LongTensor(list(gridSize)).to(self.device)
        self.units = self.aabbSize / (self.gridSize - 1)
        self.stepSize = torch.mean(self.units) * self.step_ratio
        # the same fp32 arithmetic on the host, for the world-space sampler's C argument (a device reduction may order the
        # three-term mean differently, and the sampler's bits are pinned against the host's)
        size_h = torch.tensor(self._aabb_host[3:]) - torch.tensor(self._aabb_host[:3])
        self._step_host = float(torch.mean(size_h / (torch.LongTensor(list(gridSize)) - 1)) * self.step_ratio)
        self.aabbDiag = torch.sqrt(torch.sum(torch.square(self.aabbSize)))
        self.nSamples = int((self.aabbDiag / self.stepSize).item()) + 1
        self.tSize = torch.unsqueeze(torch.tensor(tSize), 0).to(self.device)

    def init_one_svd(self, n_component, gridSize, scale, device):
        plane_coef, line_coef = [], []
        gs = [int(g) for g in gridSize]
        for i in range(3):
            vec_id = VEC_MODE[i]
            m0, m1 = MAT_MODE[i]
            p = scale * torch.randn((1, n_component[i], gs[m1], gs[m0]))
            l = scale * torch.randn((1, n_component[i], gs[vec_id], 1))
            plane_coef.append(nn.Parameter(channel_last_(p.to(device), h_fast=Z_FAST and i > 0)))
            line_coef.append(nn.Parameter(channel_last_(l.to(device))))
        return nn.ParameterList(plane_coef), nn.ParameterList(line_coef)

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        # accept planes at a different resolution (checkpoints saved after upsampling)
        for name, p in list(self.named_parameters(recurse=True)):
            key = prefix + name
            if key in state_dict and ("_plane." in name or "_line." in name) \
                    and state_dict[key].shape != p.shape:
                mod, attr = name.split(".")
                new = channel_last_(state_dict[key].to(p.device).float(),
                                    h_fast=Z_FAST and "_plane" in mod and int(attr) > 0)
                getattr(self, mod)[int(attr)] = nn.Parameter(new)
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    # ---- helpers kept from the reference API ---------------------------------------------
    def normalize_coord(self, xyz_sampled):
        return (xyz_sampled - self.aabb[0]) * self.invaabbSize - 1

    def unnormalize_coord(self, xyz_sampled):
        return (xyz_sampled + 1) / self.invaabbSize + self.aabb[0]

    def feature2density(self, density_features):
        if self.fea2denseAct == "softplus":
            return F.softplus(density_features + self.density_shift)
        return F.relu(density_features)

    def get_kwargs(self):
        return {"aabb": self.aabb, "gridSize": self.gridSize.tolist(), "tSize": self.tSize.item(),
                "density_n_comp": self.density_n_comp, "appearance_n_comp": self.app_n_comp,
                "app_dim": self.app_dim, "density_shift": self.density_shift,
                "alphaMask_thres": self.alphaMask_thres, "distance_scale": self.distance_scale,
                "rayMarch_weight_thres": self.rayMarch_weight_thres,
                "fea2denseAct": self.fea2denseAct, "near_far": self.near_far,
                "step_ratio": self.step_ratio, "shadingMode": self.shadingMode,
                "pos_pe": self.pos_pe, "view_pe": self.view_pe, "fea_pe": self.fea_pe,
                "featureC": self.featureC}

    def save(self, se3_poses, focal_ratio_refine, path):
        kwargs = self.get_kwargs()
        kwargs["se3_poses"] = se3_poses
        kwargs["focal_ratio_refine"] = focal_ratio_refine
        ckpt = {"kwargs": kwargs, "state_dict": self.state_dict()}
        if self.alphaMask is not None:   # models/tensorBase.py:465-469: shape, np.packbits payload, aabb
            from .alpha import mask_to_ckpt
            ckpt.update(mask_to_ckpt(self.alphaMask))
        torch.save(ckpt, path)

    def load(self, ckpt):
        """models/tensorBase.py:472-485; a checkpoint that carries an alpha mask rebuilds it (with the tSize the
        reference forgets to hand to AlphaGridMask), one without leaves self.alphaMask as it is."""
        if "alphaMask.aabb" in ckpt.keys():
            from .alpha import mask_from_ckpt
            self.alphaMask = mask_from_ckpt(ckpt, self.device, int(self.tSize.item()))
        self.load_state_dict(ckpt["state_dict"])

    # ---- alpha volumes and alpha-grid masks (models/tensorBase.py:565-702; alpha.py, csrc/rdrf_alpha.hip) ----------
    def compute_alpha(self, xyz_locs, t, length=1):
        from .alpha import compute_alpha
        return compute_alpha(self, xyz_locs, t, length)

    def getDenseAlpha(self, gridSize=None, times=None):
        from .alpha import get_dense_alpha
        return get_dense_alpha(self, gridSize, times)

    def updateAlphaMask(self, gridSize=(200, 200, 200)):
        from .alpha import update_alpha_mask
        return update_alpha_mask(self, gridSize)

    def filtering_rays(self, all_rays, all_rgbs, all_ts=None, N_samples=256, chunk=10240 * 5, bbox_only=False):
        from .alpha import filtering_rays
        return filtering_rays(self, all_rays, all_rgbs, all_ts, N_samples, chunk, bbox_only)

    def export_mesh(self, ply_path, t=None, level=0.005, **kw):
        """train.py:107-118 on the kernels of csrc/rdrf_iso.hip (mesh.py)"""
        from .mesh import export_mesh
        return export_mesh(self, ply_path, t, level, **kw)

    # ---- point queries (csrc/rdrf_point.hip) ---------------------------------------------------------------------------
    @torch.no_grad()
    def query_points(self, xyz, t=None, viewdirs=None, want=("sigma", "rgb"), _chunk=None):
        """The field at points off the rays: what forward() gives a sample with ray_valid = 1 at `xyz`, bit for bit, as a
        dict of tensors shaped like xyz.shape[:-1] (+ (3,) for "rgb" and "xyz_prime").

        xyz      [..., 3] un-normalised points on the device
        t        a float, or a tensor shaped xyz.shape[:-1] (a time per point).  Required for the dynamic field; the static
                 field does not read it
        viewdirs [..., 3] like xyz, or one 3-vector for all points; used AS GIVEN (forward() hands in normalised ray
                 directions).  Required exactly when "rgb" is wanted
        want     names out of "sigma" (after the density activation), "rgb" and, for the dynamic field, "blending" (after the
                 sigmoid) and "xyz_prime".  Without "rgb" no appearance kernel is launched

        Every point gets a colour: there is no weight threshold, no alpha-mask lookup and no aabb test here -- filter the
        points first where that matters.  Runs under no_grad semantics: nothing is differentiable, and inputs that require
        a gradient are detached.  Batches above the native limit (_lib.QUERY_POINTS_MAX) are queried in chunks."""
        names = ("sigma", "rgb", "blending", "xyz_prime") if self.DYNAMIC else ("sigma", "rgb")
        want = (want,) if isinstance(want, str) else tuple(want)
        bad = [w for w in want if w not in names]
        if bad:
            raise L.RdrfError(f"query_points: {bad} not among the outputs of this field, {names}")
        if not torch.is_tensor(xyz) or xyz.dim() < 1 or xyz.shape[-1] != 3:
            raise L.RdrfError("query_points: xyz must be a tensor [..., 3]")
        L.require_device(xyz)
        lead, dev = tuple(xyz.shape[:-1]), xyz.device
        pts = L.f32c(xyz.detach()).reshape(-1, 3)
        M = pts.shape[0]
        tt, per_point = None, 0
        if torch.is_tensor(t) and t.dim() > 0:
            if tuple(t.shape) != lead:
                raise L.RdrfError(f"query_points: t must be a float or shaped {lead}, not {tuple(t.shape)}")
            L.require_device(t)
            tt, per_point = L.f32c(t.detach()).reshape(-1), 1
        elif t is not None:
            tt = torch.full((1,), float(t), dtype=torch.float32, device=dev)
        if self.DYNAMIC and tt is None:
            raise L.RdrfError("query_points: the dynamic field depends on the time: pass t")
        if not self.DYNAMIC:
            tt, per_point = None, 0
        vd = None
        if "rgb" in want:
            if viewdirs is None:
                raise L.RdrfError("query_points: \"rgb\" depends on the view direction: pass viewdirs")
            v = torch.as_tensor(viewdirs, dtype=torch.float32)
            if not torch.is_tensor(viewdirs):   # a tuple or a list: host numbers, not a CPU tensor handed in by mistake
                v = v.to(dev)
            if tuple(v.shape) == (3,) and lead != ():
                v = v.expand(M, 3)
            elif tuple(v.shape) != lead + (3,):
                raise L.RdrfError(f"query_points: viewdirs must be one 3-vector or shaped {lead + (3,)}, not {tuple(v.shape)}")
            L.require_device(v)
            vd = L.f32c(v.detach()).reshape(-1, 3)
        out = {w: torch.empty((M, 3) if w in ("rgb", "xyz_prime") else (M,), device=dev) for w in want}
        chunk = int(_chunk) if _chunk else L.QUERY_POINTS_MAX
        if not 0 < chunk <= L.QUERY_POINTS_MAX:
            raise L.RdrfError(f"query_points: chunk {chunk} outside (0, {L.QUERY_POINTS_MAX}]")
        if M > 0:
            P, cfg = field_structs(self, self._param_list(), "ndc")
            dyn = int(self.DYNAMIC)
            ws = L.workspace(dev, L.lib.rdrf_query_points_ws_bytes(dyn, min(M, chunk), per_point))
            part = lambda x, a, b: L.ptr(None if x is None else x[a:b])
            for a in range(0, M, chunk):
                b = min(M, a + chunk)
                L.check(L.lib.rdrf_query_points(C.byref(P), dyn, C.byref(cfg), L.ptr(pts[a:b]), b - a,
                                                part(tt, a, b) if per_point else L.ptr(tt), per_point, part(vd, a, b),
                                                part(out.get("sigma"), a, b), part(out.get("rgb"), a, b),
                                                part(out.get("blending"), a, b), part(out.get("xyz_prime"), a, b), L.ptr(ws),
                                                ws.numel(), L.stream_of(pts)), "rdrf_query_points")
        return {w: o.view(lead + tuple(o.shape[1:])) for w, o in out.items()}

    def shrink(self, new_aabb, voxel_size=None):
        raise NotImplementedError("shrink reallocates the VM factors under the flat optimiser buffers and is not built: "
                                  "the new_aabb of updateAlphaMask is informational")

    # ---- samplers (models/tensorBase.py:487-559): device kernels, RNG stays in torch ----------
    def sample_ray_ndc(self, rays_o, rays_d, is_train=True, N_samples=-1):
        from .renderer import sample_rays
        N_samples = N_samples if N_samples > 0 else self.nSamples
        xyz, z, valid = sample_rays(self, torch.cat([rays_o, rays_d], -1), N_samples, "ndc", is_train)
        return xyz, z[:1], valid

    def sample_ray_contracted(self, rays_o, rays_d, is_train=True, N_samples=-1):
        from .renderer import sample_rays
        N_samples = N_samples if N_samples > 0 else self.nSamples
        xyz, z, valid = sample_rays(self, torch.cat([rays_o, rays_d], -1), N_samples, "contract",
                                    is_train)
        return xyz, z[:1], valid

    def sample_ray(self, rays_o, rays_d, is_train=True, N_samples=-1):
        """models/tensorBase.py:501-522: the world-space march; z_vals per ray, [N,S]"""
        from .renderer import sample_rays
        N_samples = N_samples if N_samples > 0 else self.nSamples
        return sample_rays(self, torch.cat([rays_o, rays_d], -1), N_samples, "world", is_train)

    @torch.no_grad()
    def up_sampling_VM(self, plane_coef, line_coef, res_target):
        """models/tensoRF.py:199-221 / 814-836: bilinear (align_corners) resampling of a factor family to
        the new grid -- rdrf_upsample_bilinear, one launch for the six tensors, channel-last in and out."""
        srcs, dsts = [], []
        for i in range(3):
            vec_id = VEC_MODE[i]
            m0, m1 = MAT_MODE[i]
            p, l = plane_coef[i].data, line_coef[i].data
            L.require_device(p, l)
            newp = torch.empty((1, p.shape[1], int(res_target[m1]), int(res_target[m0])), device=p.device)
            newl = torch.empty((1, l.shape[1], int(res_target[vec_id]), 1), device=l.device)
            newp, newl = channel_last_(newp, h_fast=Z_FAST and i > 0), channel_last_(newl)
            srcs += [p, l]
            dsts += [newp, newl]
        sa = (L.RdrfTensor4 * 6)(*[_tensor4(t) for t in srcs])
        da = (L.RdrfTensor4 * 6)(*[_tensor4(t) for t in dsts])
        L.check(L.lib.rdrf_upsample_bilinear(sa, da, 6, L.stream_of(srcs[0])), "rdrf_upsample_bilinear")
        for i in range(3):
            plane_coef[i] = nn.Parameter(dsts[2 * i])
            line_coef[i] = nn.Parameter(dsts[2 * i + 1])
        return plane_coef, line_coef

    # ---- fused gradient accumulation ----------------------------------------------------
    # The C ABI accumulates (+=) into caller-owned gradient buffers.  With `fused_grad` on, every
    # backward pass of this field adds straight into p.grad, and all p.grad are views of ONE flat
    # fp32 buffer: a step costs one memset instead of ~40 zeros_like + ~40 autograd adds per pass
    # (rocprofv3: 413 fill + 230 add launches, 2.3 ms, per 5-pass step), and the data-parallel
    # exchange all-reduces the flat buffer in place.  Off by default: plain autograd semantics
    # (torch.autograd.grad, retain_graph, ...) need freshly returned gradients.
    fused_grad = False
    DYNAMIC = False    # which parameter struct and entry points this field takes (_params.field_structs)
    _pack_epoch = 0    # bumped by whoever writes the parameters through raw pointers (optim.FlatAdam): see _attach_packed

    @property
    def pack_cache(self):
        """whether _params._attach_packed keeps packed weight images for this field: the module switch PACK_CACHE, read per call"""
        return PACK_CACHE

    def invalidate_packed(self):
        """Drop the cached packed weight images.  Needed only after an MLP weight was edited in a way torch's version
        counters do not see: through `.data`, or through raw pointers (optim.FlatAdam does it itself)."""
        self._pack_epoch += 1

    FLAT_ALIGN = 4096   # floats: the flat buffers split evenly over 1, 2, 4, 8 ... ranks in 16-byte units

    def _flat_layout(self):
        """(offsets, total, split): float offset of every parameter of _param_list() inside the flat
        buffers (64-float aligned), the padded total, and the offset where the VM factors end and the
        networks begin (the two learning rates of get_optparam_groups)."""
        params = self._param_list()
        offs, total = [], 0
        for p in params:
            offs.append(total)
            total += (p.numel() + 63) // 64 * 64
        n_vm = sum(1 for n, _ in self.named_parameters() if "_plane." in n or "_line." in n)
        split = offs[n_vm] if n_vm < len(offs) else total
        total = (total + self.FLAT_ALIGN - 1) // self.FLAT_ALIGN * self.FLAT_ALIGN
        return offs, total, split

    def fused_grads(self):
        params = self._param_list()
        views = getattr(self, "_gviews", None)
        ok = views is not None and len(views) == len(params) and all(
            p.grad is not None and p.grad.data_ptr() == v.data_ptr() and p.grad.stride() == v.stride()
            and p.shape == v.shape for p, v in zip(params, views))
        if not ok:
            offs, total, _ = self._flat_layout()
            flat = torch.zeros(total, dtype=torch.float32, device=params[0].device)
            views = [torch.as_strided(flat, p.size(), p.stride(), o) for p, o in zip(params, offs)]
            with torch.no_grad():
                for p, v in zip(params, views):
                    if p.grad is not None and p.grad.shape == v.shape:
                        v.copy_(p.grad)
                    p.grad = v
            self._gflat, self._gviews = flat, views
            self._det_shadow = torch.zeros(total, dtype=torch.int64, device=flat.device) if L.DETERMINISTIC else None
        return views

    # ---- deterministic debugging build (RDRF_DETERMINISTIC=1, librodynrf_det.so) -----------------------------------------
    def _det_bind(self):
        """bind this field's flat gradient buffer to its fixed-point shadow for the backward about to run"""
        if not L.DETERMINISTIC:
            return
        if not self.fused_grad:
            raise L.RdrfError("RDRF_DETERMINISTIC=1 needs the fused gradient buffers (field.fused_grad = True): only additions "
                              "into a bound flat buffer are order-independent")
        self.fused_grads()
        L.check(L.lib.rdrf_det_bind(int(self.DYNAMIC), L.ptr(self._gflat), self._gflat.numel(), L.ptr(self._det_shadow),
                                    L.stream_of(self._gflat)), "rdrf_det_bind")

    def det_fold_(self):
        """fold the fixed-point shadow into the fp32 gradients (call before anything reads .grad); no-op otherwise"""
        if L.DETERMINISTIC and getattr(self, "_det_shadow", None) is not None:
            self._det_bind()
            L.check(L.lib.rdrf_det_finish(int(self.DYNAMIC), L.stream_of(self._gflat)), "rdrf_det_finish")

    def flatten_params_(self):
        """Make every parameter a view of ONE flat fp32 buffer (same layout as the fused gradient buffer):
        the Adam kernel then updates a field with one launch over (p, g, m, v) flat ranges, and the
        sharded data-parallel step reduce-scatters / all-gathers the flat buffers in place.  Values,
        shapes, strides and state_dict() are unchanged.  Returns the flat buffer (idempotent)."""
        params = self._param_list()
        offs, total, _ = self._flat_layout()
        flat = getattr(self, "_pflat", None)
        ok = flat is not None and flat.numel() == total and all(
            p.data_ptr() == flat.data_ptr() + 4 * o for p, o in zip(params, offs))
        if not ok:
            flat = torch.zeros(total, dtype=torch.float32, device=params[0].device)
            with torch.no_grad():
                for p, o in zip(params, offs):
                    v = torch.as_strided(flat, p.size(), p.stride(), o)
                    v.copy_(p.data)
                    p.data = v
            self._pflat = flat
        return flat

    def zero_grad_fused(self):
        """one memset for every gradient of this field (replaces optimizer.zero_grad())"""
        self.fused_grads()
        self._gflat.zero_()
        if getattr(self, "_det_shadow", None) is not None:
            self._det_shadow.zero_()
        return self._gflat

    def _check_layout(self):
        for n, p in self.named_parameters():
            if ("_plane." in n or "_line." in n) and not _is_channel_last(p):
                raise L.RdrfError(f"{n} lost its channel-last layout")


def query_points(field, xyz, t=None, viewdirs=None, want=("sigma", "rgb")):
    """field.query_points(xyz, t, viewdirs, want): see TensorBase.query_points"""
    return field.query_points(xyz, t, viewdirs, want)


class TensorVMSplit(TensorBase):
    """Static field (models/tensoRF.py:11-274)."""

    def init_svd_volume(self, res, device):
        self.density_plane, self.density_line = self.init_one_svd(self.density_n_comp, self.gridSize,
                                                                  0.1, device)
        self.app_plane, self.app_line = self.init_one_svd(self.app_n_comp, self.gridSize, 0.1, device)
        self.basis_mat = nn.Linear(sum(self.app_n_comp), self.app_dim, bias=False).to(device)

    def get_optparam_groups(self, lr_init_spatialxyz=0.02, lr_init_network=0.001):
        return [{"params": self.density_line, "lr": lr_init_spatialxyz},
                {"params": self.density_plane, "lr": lr_init_spatialxyz},
                {"params": self.app_line, "lr": lr_init_spatialxyz},
                {"params": self.app_plane, "lr": lr_init_spatialxyz},
                {"params": self.basis_mat.parameters(), "lr": lr_init_network},
                {"params": self.renderModule.parameters(), "lr": lr_init_network}]

    def _param_list(self):
        rm = self.renderModule
        if self.shadingMode == "MLP_Fea":
            if self.fea_pe != 2:
                raise NotImplementedError("static MLP_Fea head is built for fea_pe=2 (train.py:889)")
            last = rm.mlp[4]
        elif self.shadingMode == "MLP_Fea_TimeEmbedding":
            if self.fea_pe != 2:
                raise NotImplementedError("static head is built for fea_pe=2 (train.py:889)")
            last = rm.mlp_view[0]
        else:
            raise NotImplementedError("static field heads: MLP_Fea | MLP_Fea_TimeEmbedding")
        return (list(self.density_plane) + list(self.density_line) + list(self.app_plane)
                + list(self.app_line) + [self.basis_mat.weight, rm.mlp[0].weight, rm.mlp[0].bias,
                                         rm.mlp[2].weight, rm.mlp[2].bias, last.weight, last.bias])

    def warp_coordinate(self, xyz_sampled, t_sampled):
        return None

    # ---- models/tensoRF.py:118-196: the per-point building blocks of forward() -------------------
    def compute_densityfeature(self, xyz_sampled, t_sampled=None, time_embedding_sampled=None):
        """xyz_sampled [M,3] NORMALISED coordinates -> sigma feature [M] (sum of the 24 VM products,
        before feature2density).  t_sampled / time_embedding_sampled are accepted and unused, as in
        the reference.  Differentiable wrt the density factors and the coordinates."""
        return _StaticFeatFn.apply(self, torch.is_grad_enabled(), True, False, xyz_sampled.reshape(-1, 3), *self._param_list())[0]

    def compute_appfeature(self, xyz_sampled, t_sampled=None, time_embedding_sampled=None):
        """xyz_sampled [M,3] normalised -> basis_mat(72 VM products) [M,27]"""
        return _StaticFeatFn.apply(self, torch.is_grad_enabled(), False, True, xyz_sampled.reshape(-1, 3), *self._param_list())[1]

    # models/tensoRF.py:63-98
    def vectorDiffs(self, vector_comps):
        return vector_diffs(vector_comps)

    def vector_comp_diffs(self):
        return vector_diffs(self.density_line) + vector_diffs(self.app_line)

    def density_L1(self):
        return dense_l1(self, self.density_plane, self.density_line)

    # models/tensoRF.py:100-116
    def TV_loss_density(self, reg):
        return tv_family(self, reg, self.density_plane, self.density_line)

    def TV_loss_app(self, reg):
        return tv_family(self, reg, self.app_plane, self.app_line)

    def forward(self, rays_chunk, ts_chunk, timeembeddings_chunk, xyz_sampled, z_vals, ray_valid,
                white_bg=True, is_train=False, ray_type="ndc", N_samples=-1, rgb=True):
        """rgb=False (extension): the caller does not consume the colours (entry 6 of the tuple is None) and the
        appearance phase -- gather, basis, RGB head: ~70 % of this field's forward work -- is not run.
        rgb="value": the colours are computed and returned bit-identically, but as values only (not differentiable): the
        appearance phase runs the inference kernel and saves no rows -- rows are saved only where a backward can read them.
        Under torch.no_grad() no backward can exist and nothing at all is saved."""
        if timeembeddings_chunk is not None:
            raise NotImplementedError("timeembeddings_chunk is None at every reference call site")
        rgb, sigma, weight, dists = _StaticFn.apply(self, ray_type, *_call_modes(rgb), rays_chunk, ts_chunk,
                                                    xyz_sampled, z_vals, ray_valid, *self._param_list())
        return FieldOut(None, None, None, xyz_sampled, weight, None, rgb, sigma, z_vals, dists)

    @torch.no_grad()
    def upsample_volume_grid(self, res_target):
        self.app_plane, self.app_line = self.up_sampling_VM(self.app_plane, self.app_line, res_target)
        self.density_plane, self.density_line = self.up_sampling_VM(self.density_plane,
                                                                    self.density_line, res_target)
        self.update_stepSize(res_target, 1)


class TensorVMSplit_TimeEmbedding(TensorBase):
    """Dynamic field (models/tensoRF.py:277-892)."""
    DYNAMIC = True

    def __init__(self, aabb, gridSize, tSize, device, **kargs):
        super().__init__(aabb, gridSize, tSize, device, **kargs)
        self.layer1 = nn.Linear(1 + 8 * 2 * 1, 64).to(device)
        self.layer2 = nn.Linear(64, 30).to(device)
        self.layer3 = nn.Linear((3 + 10 * 2 * 3) + 30, 64).to(device)
        self.layer4 = nn.Linear(64, 64).to(device)
        self.layer5 = nn.Linear(64, 3).to(device)
        nin = sum(self.density_n_comp) * 3 + 3 + 10 * 2 * 3 + 1 + 8 * 2 * 1
        self.density_layer1 = nn.Linear(nin, 64).to(device)
        self.density_layer2 = nn.Linear(64, 1).to(device)
        self.blending_layer1 = nn.Linear(nin, 64).to(device)
        self.blending_layer2 = nn.Linear(64, 1).to(device)
        self.scene_flow_mlp = nn.Sequential(
            nn.Linear(4 * 2 * 4 + 4, 64), nn.ReLU(inplace=True), nn.Linear(64, 64),
            nn.ReLU(inplace=True), nn.Linear(64, 64), nn.ReLU(inplace=True), nn.Linear(64, 6),
        ).to(device)
        if self.shadingMode != "MLP_Fea_late_view" or self.fea_pe != 0:
            raise NotImplementedError("dynamic head is built for MLP_Fea_late_view, fea_pe=0 "
                                      "(configs/*.txt, train.py:918)")

    def init_svd_volume(self, res, device):
        self.blending_plane, self.blending_line = self.init_one_svd(self.density_n_comp,
                                                                    self.gridSize, 0.1, device)
        self.density_plane, self.density_line = self.init_one_svd(self.density_n_comp, self.gridSize,
                                                                  0.1, device)
        self.app_plane, self.app_line = self.init_one_svd(self.app_n_comp, self.gridSize, 0.1, device)
        self.basis_mat = nn.Linear(sum(self.app_n_comp) * 3, self.app_dim, bias=False).to(device)

    def get_optparam_groups(self, lr_init_spatialxyz=0.02, lr_init_network=0.001):
        g = [{"params": self.density_line, "lr": lr_init_spatialxyz},
             {"params": self.density_plane, "lr": lr_init_spatialxyz},
             {"params": self.blending_line, "lr": lr_init_spatialxyz},
             {"params": self.blending_plane, "lr": lr_init_spatialxyz},
             {"params": self.app_line, "lr": lr_init_spatialxyz},
             {"params": self.app_plane, "lr": lr_init_spatialxyz},
             {"params": self.basis_mat.parameters(), "lr": lr_init_network},
             {"params": self.scene_flow_mlp.parameters(), "lr": lr_init_network}]
        for m in (self.layer1, self.layer2, self.layer3, self.layer4, self.layer5, self.density_layer1,
                  self.density_layer2, self.blending_layer1, self.blending_layer2):
            g.append({"params": m.parameters(), "lr": lr_init_network})
        g.append({"params": self.renderModule.parameters(), "lr": lr_init_network})
        return g

    def _param_list(self):
        rm = self.renderModule
        t = (list(self.density_plane) + list(self.density_line) + list(self.blending_plane)
             + list(self.blending_line) + list(self.app_plane) + list(self.app_line))
        t += [self.basis_mat.weight, rm.mlp[0].weight, rm.mlp[0].bias, rm.mlp[2].weight,
              rm.mlp[2].bias, rm.mlp_view[0].weight, rm.mlp_view[0].bias]
        for m in (self.layer1, self.layer2, self.layer3, self.layer4, self.layer5, self.density_layer1,
                  self.density_layer2, self.blending_layer1, self.blending_layer2):
            t += [m.weight, m.bias]
        for i in (0, 2, 4, 6):
            t += [self.scene_flow_mlp[i].weight, self.scene_flow_mlp[i].bias]
        return t

    def forward(self, rays_chunk, ts_chunk, timeembeddings_chunk, xyz_sampled, z_vals, ray_valid,
                white_bg=True, is_train=False, ray_type="ndc", N_samples=-1, rgb=True):
        """rgb=False | "value" (extension): see TensorVMSplit.forward"""
        if timeembeddings_chunk is not None:
            raise NotImplementedError("timeembeddings_chunk is None at every reference call site")
        blending, weight, xyz_prime, rgb, sigma, dists = _DynamicFn.apply(
            self, ray_type, *_call_modes(rgb), rays_chunk, ts_chunk, xyz_sampled, z_vals, ray_valid,
            *self._param_list())
        return FieldOut(None, None, blending, xyz_sampled, weight, xyz_prime, rgb, sigma, z_vals, dists)

    # models/tensoRF.py:378-416 (the reference's dynamic class has no vector_comp_diffs)
    def density_L1(self):
        return dense_l1(self, self.density_plane, self.density_line)

    def blending_L1(self):
        return dense_l1(self, self.blending_plane, self.blending_line)

    # models/tensoRF.py:418-444
    def TV_loss_blending(self, reg):
        return tv_family(self, reg, self.blending_plane, self.blending_line)

    def TV_loss_density(self, reg):
        return tv_family(self, reg, self.density_plane, self.density_line)

    def TV_loss_app(self, reg):
        return tv_family(self, reg, self.app_plane, self.app_line)

    def get_forward_backward_scene_flow(self, unnormalized_pts, t_sampled):
        return _SceneFlowFn.apply(self, torch.is_grad_enabled(), unnormalized_pts, t_sampled, *self._param_list())

    def get_forward_backward_scene_flow_point_single(self, pts_map_NDC, t_sampled):
        """models/tensoRF.py:506-519: one point per ray, pts_map_NDC [N,3] un-normalised, t_sampled [N] ->
        (pts + scene_flow_f, pts + scene_flow_b, scene_flow_f, scene_flow_b), each [N,3].  The S = 1 case of
        get_forward_backward_scene_flow: the same kernel, the same bits, the same backward."""
        if pts_map_NDC.dim() != 2 or pts_map_NDC.shape[-1] != 3 or t_sampled.shape != pts_map_NDC.shape[:1]:
            raise L.RdrfError("get_forward_backward_scene_flow_point_single: expected pts_map_NDC [N,3] and t_sampled [N]")
        sf_f, sf_b = self.get_forward_backward_scene_flow(pts_map_NDC.reshape(-1, 1, 3), t_sampled)
        sf_f, sf_b = sf_f.reshape(-1, 3), sf_b.reshape(-1, 3)
        return pts_map_NDC + sf_f, pts_map_NDC + sf_b, sf_f, sf_b

    def _features(self, want, x, t, normalized):
        x2 = x.reshape(-1, 3)
        t2 = t.reshape(-1)
        if t2.numel() != x2.shape[0]:
            raise L.RdrfError(f"compute_*: {x2.shape[0]} points but {t2.numel()} times")
        return _DynFeatFn.apply(self, torch.is_grad_enabled(), want, normalized, x2, t2, *self._param_list())

    def warp_coordinate(self, unnormalized_xyz_sampled, t_sampled):
        """models/tensoRF.py:521-541: (...,3) un-normalised points, (...) times -> warped un-normalised
        points, same shape.  Differentiable wrt the warp MLP, the coordinates (not the times)."""
        out = self._features(("warp",), unnormalized_xyz_sampled, t_sampled, False)[3]
        return out.reshape(unnormalized_xyz_sampled.shape)

    def compute_densityfeature(self, xyz_sampled, t_sampled, time_embedding_sampled=None):
        """models/tensoRF.py:646-732: xyz_sampled [M,3] NORMALISED, t_sampled [M] -> density_layer2 output [M]
        (3-stride VM features at the warped point + [xn, PE10, t, PE8] -> 64 -> 1)."""
        return self._features(("density",), xyz_sampled, t_sampled, True)[0]

    def compute_blendingfeature(self, xyz_sampled, t_sampled, time_embedding_sampled=None):
        """models/tensoRF.py:543-629 (before the sigmoid)"""
        return self._features(("blending",), xyz_sampled, t_sampled, True)[1]

    def compute_appfeature(self, xyz_sampled, t_sampled, time_embedding_sampled=None):
        """models/tensoRF.py:734-811: basis_mat(216 3-stride VM features at the warped point) [M,27]"""
        return self._features(("app",), xyz_sampled, t_sampled, True)[2]

    @torch.no_grad()
    def upsample_volume_grid(self, res_target):
        self.app_plane, self.app_line = self.up_sampling_VM(self.app_plane, self.app_line, res_target)
        self.density_plane, self.density_line = self.up_sampling_VM(self.density_plane,
                                                                    self.density_line, res_target)
        self.blending_plane, self.blending_line = self.up_sampling_VM(self.blending_plane,
                                                                      self.blending_line, res_target)
        self.update_stepSize(res_target, 1)
