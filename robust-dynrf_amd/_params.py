"""The parameter and cfg structs of the C ABI (include/rodynrf.h RdrfVM, RdrfFieldCfg, RdrfStaticParams,
RdrfDynamicParams) built from the field objects, and the packed weight images that ride in them.  Imports only `_lib`, so
fields, renderer, alpha and regularizers all take the builders from here."""
import ctypes as C

import torch

from . import _lib as L


def _vm_struct(planes, lines):
    vm = L.RdrfVM()
    for i in range(3):
        p, l = planes[i], lines[i]
        # the kernels read components with stride 1 (16-byte quads) and lines as [L][C]: a factor that
        # lost its channel-last storage (user-assigned parameter, .contiguous(), external resampling)
        # would be read with the wrong layout -- fail loudly instead
        if p.stride(1) != 1 or l.stride(1) != 1 or l.stride(2) != l.shape[1] or p.shape[1] % 4 != 0:
            raise L.RdrfError(f"VM factor {i} is not channel-last (plane strides {tuple(p.stride())}, line strides "
                              f"{tuple(l.stride())}): use fields.channel_last_()")
        vm.plane[i] = p.data_ptr()
        vm.line[i] = l.data_ptr()
        vm.C[i] = p.shape[1]
        vm.H[i] = p.shape[2]
        vm.W[i] = p.shape[3]
        vm.L[i] = l.shape[2]
        vm.sH[i] = p.stride(2)
        vm.sW[i] = p.stride(3)
    return vm


def _cfg_struct(field, ray_type, weight_thres=None):
    c = L.RdrfFieldCfg()
    ab = field._aabb_host
    for i in range(6):
        c.aabb[i] = ab[i]
    c.distance_scale = float(field.distance_scale)
    c.weight_thres = float(field.rayMarch_weight_thres if weight_thres is None else weight_thres)
    c.density_shift = float(field.density_shift)
    c.act = L.ACTS[field.fea2denseAct]
    c.ray_type = L.RAY_TYPES.get(ray_type, 2)
    c.static_head = L.HEADS.get(field.shadingMode, 0)
    return c


def _static_struct(t):
    """t: list of tensors in TensorVMSplit._param_list() order."""
    P = L.RdrfStaticParams()
    P.density = _vm_struct(t[0:3], t[3:6])
    P.app = _vm_struct(t[6:9], t[9:12])
    for name, ten in zip(("basis", "w1", "b1", "w2", "b2", "w3", "b3"), t[12:19]):
        setattr(P, name, ten.data_ptr())
    return P


def _dynamic_struct(t):
    P = L.RdrfDynamicParams()
    P.density = _vm_struct(t[0:3], t[3:6])
    P.blending = _vm_struct(t[6:9], t[9:12])
    P.app = _vm_struct(t[12:15], t[15:18])
    names = ("basis", "rw1", "rb1", "rw2", "rb2", "rwv", "rbv", "l1w", "l1b", "l2w", "l2b", "l3w",
             "l3b", "l4w", "l4b", "l5w", "l5b", "dw1", "db1", "dw2", "db2", "bw1", "bb1", "bw2", "bb2")
    for name, ten in zip(names, t[18:43]):
        setattr(P, name, ten.data_ptr())
    for i in range(4):
        P.sfw[i] = t[43 + 2 * i].data_ptr()
        P.sfb[i] = t[44 + 2 * i].data_ptr()
    return P


# Packed weight images (rdrf_static_pack / rdrf_dynamic_pack): the MLP weights of a field do not change between the
# passes of an iteration or the chunks of a render, so the image is packed once per (weights, stream) and handed to
# the entry points through packed_fwd / packed_bwd instead of being re-packed by every call (~40 launches of ~6 us
# per training iteration).  The key is every MLP tensor's (data_ptr, torch version counter) plus the field's
# `_pack_epoch`, which optim.FlatAdam bumps because rdrf_adam_step writes the parameters through raw pointers.
# The switch is the field's: `field.pack_cache` (fields.PACK_CACHE, RDRF_PACK_CACHE=0 turns the images off).
def _attach_packed(field, P, params, backward, dynamic):
    if field is None or not field.pack_cache:
        return
    first = 18 if dynamic else 12
    stream = torch.cuda.current_stream(params[0].device).cuda_stream
    key = (tuple((p.data_ptr(), p._version) for p in params[first:]), field._pack_epoch)
    cache = field.__dict__.setdefault("_pack_cache", {})
    # one image per (direction, stream): a re-pack into an image is ordered behind that stream's earlier readers;
    # another stream gets its own image instead of racing with kernels still reading this one
    slot = cache.get((backward, stream))
    if slot is None or slot[0] != key:
        img = slot[1] if slot is not None else torch.empty(int(L.lib.rdrf_pack_floats()), device=params[0].device)
        if dynamic:
            L.check(L.lib.rdrf_dynamic_pack(C.byref(P), int(backward), L.ptr(img), stream), "rdrf_dynamic_pack")
        else:
            L.check(L.lib.rdrf_static_pack(C.byref(P), L.HEADS.get(field.shadingMode, 0), int(backward), L.ptr(img), stream),
                    "rdrf_static_pack")
        cache[(backward, stream)] = slot = (key, img)
    if backward:
        P.packed_bwd = slot[1].data_ptr()
    else:
        P.packed_fwd = slot[1].data_ptr()


def field_structs(field, params, ray_type, backward=False):
    """What every field entry point takes first: (the parameter struct of `params` with the packed image of that direction
    attached, the cfg).  `field.DYNAMIC` says which of the two structs; `params` is field._param_list() or the tensors an
    autograd Function saved of it."""
    P = (_dynamic_struct if field.DYNAMIC else _static_struct)(params)
    _attach_packed(field, P, params, backward, field.DYNAMIC)
    return P, _cfg_struct(field, ray_type)


def render_structs(tensorf_static, tensorf, ray_type):
    """(PS, cs, PD, cd) of the render entry points; the images are packed once per (weights, stream), on the current
    stream, not per chunk"""
    return (*field_structs(tensorf_static, tensorf_static._param_list(), ray_type),
            *field_structs(tensorf, tensorf._param_list(), ray_type))
