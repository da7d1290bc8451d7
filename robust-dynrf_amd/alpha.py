"""Dense alpha volumes and alpha-grid masks (the reference's models/tensorBase.py:42-79 AlphaGridMask, :565-702
compute_alpha / getDenseAlpha / updateAlphaMask / filtering_rays) on the kernels of csrc/rdrf_alpha.hip.

The occupancy grid lives on the device bit-packed exactly as the reference's `save` stores it (np.packbits of the bool
volume of logical shape (G2, G1, G0, T)): the buffer is the checkpoint payload, and the sampling kernel interpolates
straight from the bits.  `TensorBase` (fields.py) exposes the functions here as its methods.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from ._params import field_structs

SLAB_POINTS = 1 << 21   # lattice points per native alpha call of getDenseAlpha (a bound on what one launch holds busy)

_BIT_WEIGHTS = (128, 64, 32, 16, 8, 4, 2, 1)


def pack_bits(volume):
    """np.packbits(volume.reshape(-1)) for a bool tensor, on its device"""
    flat = volume.reshape(-1).to(torch.uint8)
    pad = (-flat.numel()) % 8
    if pad:
        flat = torch.cat([flat, flat.new_zeros(pad)])
    w = torch.tensor(_BIT_WEIGHTS, dtype=torch.uint8, device=flat.device)
    return (flat.view(-1, 8) * w).sum(1, dtype=torch.int32).to(torch.uint8)


def unpack_bits(packed, count):
    """np.unpackbits(packed)[:count] as a bool tensor, on its device"""
    sh = torch.arange(7, -1, -1, dtype=torch.uint8, device=packed.device)
    return ((packed.view(-1, 1) >> sh) & 1).reshape(-1)[:count].bool()


class AlphaGridMask:
    """models/tensorBase.py:42-79: AlphaGridMask(device, aabb, alpha_volume, tSize) with alpha_volume of shape
    (G2, G1, G0, T) (the reference stores 0 / 1 floats; anything non-zero is occupied).  Attributes as in
    the reference: aabb, aabbSize, invgridSize, gridSize (LongTensor [G0, G1, G2]), tSize, and alpha_volume -- a float view
    (1, 1, G2, G1, G0, T) unpacked on demand.  `packed` is the storage: uint8 on the device."""

    def __init__(self, device, aabb, alpha_volume, tSize):
        vol = torch.as_tensor(alpha_volume)
        shape = tuple(int(v) for v in vol.shape[:3])
        self._init(device, aabb, pack_bits(vol.reshape(*shape, int(tSize)) != 0), shape, tSize)

    @classmethod
    def from_packed(cls, device, aabb, packed, shape, tSize):
        """packed: uint8 tensor / array in the checkpoint's layout; shape: (G2, G1, G0)"""
        self = cls.__new__(cls)
        self._init(device, aabb, torch.as_tensor(np.asarray(packed) if not torch.is_tensor(packed) else packed), shape, tSize)
        return self

    def _init(self, device, aabb, packed, shape, tSize):
        self.device = device
        self.aabb = torch.as_tensor(aabb, dtype=torch.float32).to(device)
        self.aabbSize = self.aabb[1] - self.aabb[0]
        self.invgridSize = 1.0 / self.aabbSize * 2
        self.tSize = int(tSize)
        self._shape = tuple(int(v) for v in shape)   # (G2, G1, G0)
        self.gridSize = torch.LongTensor([self._shape[2], self._shape[1], self._shape[0]]).to(device)
        count = self._shape[0] * self._shape[1] * self._shape[2] * self.tSize
        packed = packed.reshape(-1).to(torch.uint8)
        if packed.numel() != (count + 7) // 8:
            raise L.RdrfError(f"AlphaGridMask: {packed.numel()} packed bytes for a volume of {self._shape + (self.tSize,)}")
        self.packed = packed.to(device).contiguous()
        self._aabb_host = [float(v) for v in self.aabb.detach().cpu().reshape(-1)]

    @property
    def shape(self):
        """the checkpoint's "alphaMask.shape\""""
        return (1, 1) + self._shape + (self.tSize,)

    @property
    def alpha_volume(self):
        n = int(np.prod(self.shape))
        return unpack_bits(self.packed, n).float().view(self.shape)

    def _struct(self):
        L.require_device(self.packed)
        m = L.RdrfAlphaMask()
        m.bits = self.packed.data_ptr()
        m.grid[0], m.grid[1], m.grid[2] = self._shape[2], self._shape[1], self._shape[0]
        m.T = self.tSize
        for i in range(6):
            m.aabb[i] = self._aabb_host[i]
        return m

    def normalize_coord(self, xyz_sampled):
        return (xyz_sampled - self.aabb[0]) * self.invgridSize - 1

    def sample_alpha(self, xyz_sampled, t):
        """-> [n] trilinear samples of the slice round((t + 1) / 2 (tSize - 1)); t: a scalar or one value per point"""
        L.require_device(xyz_sampled)
        xyz = L.f32c(xyz_sampled).reshape(-1, 3)
        n = xyz.shape[0]
        tt = torch.as_tensor(t, dtype=torch.float32, device=xyz.device).reshape(-1)
        if tt.numel() not in (1, n):
            raise L.RdrfError(f"sample_alpha: {n} points but {tt.numel()} times")
        tt = tt.contiguous()
        out = torch.empty(n, device=xyz.device)
        m = self._struct()
        L.check(L.lib.rdrf_alpha_mask_sample(C.byref(m), L.ptr(xyz), L.ptr(tt), int(tt.numel() == n and n > 1), n, L.ptr(out),
                                             L.stream_of(xyz)), "rdrf_alpha_mask_sample")
        return out


def apply_alpha_mask(valid, xyz, ts, *masks):
    """`ray_valid &= alpha_mask` (models/tensorBase.py:746-752) for xyz [N,S,3], ts [N]: the filtered copy of `valid`, kept
    where the sample of ANY of the (one or two) masks is > 0.  Hand the result to the fields' forward as ray_valid."""
    masks = [m for m in masks if m is not None]
    if not masks:
        return valid
    if len(masks) > 2:
        raise L.RdrfError("apply_alpha_mask takes at most two masks")
    L.require_device(valid, xyz, ts)
    N, S = valid.shape
    out = valid.contiguous().clone()
    v8 = out.view(torch.uint8) if out.dtype == torch.bool else out
    xyz, ts = L.f32c(xyz), L.f32c(ts).reshape(-1)
    if xyz.numel() != N * S * 3 or ts.numel() != N:
        raise L.RdrfError(f"apply_alpha_mask: valid {tuple(valid.shape)}, xyz {tuple(xyz.shape)}, ts {tuple(ts.shape)}")
    m0 = masks[0]._struct()
    m1 = masks[1]._struct() if len(masks) == 2 else None
    L.check(L.lib.rdrf_alpha_mask_valid(C.byref(m0), C.byref(m1) if m1 is not None else None, L.ptr(xyz), L.ptr(ts), N, S,
                                        L.ptr(v8), L.stream_of(xyz)), "rdrf_alpha_mask_valid")
    return out


def alpha_volume(field, xyz, times, length, mask=None, want_sigma=False, out=None):
    """rdrf_compute_alpha: xyz [M,3] un-normalised, times [T] -> alpha [M,T] (and sigma [M,T])"""
    L.require_device(xyz, times)
    xyz, times = L.f32c(xyz).reshape(-1, 3), L.f32c(times).reshape(-1)
    M, T = xyz.shape[0], times.numel()
    dev = xyz.device
    alpha = torch.empty(M, T, device=dev) if out is None else out
    sigma = torch.empty(M, T, device=dev) if want_sigma else None
    P, cfg = field_structs(field, field._param_list(), "ndc")
    ws = L.workspace(dev, L.lib.rdrf_compute_alpha_workspace_bytes(M, T))
    m = mask._struct() if mask is not None else None
    L.check(L.lib.rdrf_compute_alpha(C.byref(P), int(field.DYNAMIC), C.byref(cfg), L.ptr(xyz), M, L.ptr(times), T, float(length),
                                     C.byref(m) if m is not None else None, L.ptr(alpha), L.ptr(sigma), L.ptr(ws),
                                     ws.numel(), L.stream_of(xyz)), "rdrf_compute_alpha")
    return (alpha, sigma) if want_sigma else alpha


@torch.no_grad()
def compute_alpha(field, xyz_locs, t, length=1):
    """models/tensorBase.py:684-702 as it is meant (the reference passes two of compute_densityfeature's three arguments):
    alpha = 1 - exp(-sigma length) at un-normalised points; points the field's alphaMask leaves empty get 0.
    t a scalar -> alpha of xyz_locs.shape[:-1]; t a 1-D tensor of T times -> [..., T]."""
    tt = torch.as_tensor(t, dtype=torch.float32, device=xyz_locs.device)
    a = alpha_volume(field, xyz_locs, tt.reshape(-1), float(length), field.alphaMask)
    lead = tuple(xyz_locs.shape[:-1])
    return a.view(lead) if tt.dim() == 0 else a.view(lead + (tt.numel(),))


def lattice_times(tSize):
    if tSize < 2:
        raise ValueError(f"the alpha volume takes its times from k / (tSize - 1) * 2 - 1: tSize must be at least 2, not {tSize}")
    return torch.tensor([k / (tSize - 1.0) * 2.0 - 1.0 for k in range(tSize)], dtype=torch.float32)


def _dense_lattice(field, gridSize, times):
    """the lattice of getDenseAlpha over field.aabb -> (gs, times [T] on the device, dense_xyz [G0,G1,G2,3], the slabs
    (i0, i1) of G0 that hold at most SLAB_POINTS points each)"""
    gs = [int(v) for v in (field.gridSize.tolist() if gridSize is None else gridSize)]
    dev = field.aabb.device
    times = lattice_times(int(field.tSize.item())) if times is None else torch.as_tensor(times, dtype=torch.float32).reshape(-1)
    times = times.to(dev)
    samples = torch.stack(torch.meshgrid(torch.linspace(0, 1, gs[0], device=dev), torch.linspace(0, 1, gs[1], device=dev),
                                         torch.linspace(0, 1, gs[2], device=dev), indexing="ij"), -1)
    dense_xyz = field.aabb[0] * (1 - samples) + field.aabb[1] * samples
    rows = max(1, SLAB_POINTS // (gs[1] * gs[2]))
    return gs, times, dense_xyz, [(i0, min(gs[0], i0 + rows)) for i0 in range(0, gs[0], rows)]


@torch.no_grad()
def get_dense_alpha(field, gridSize=None, times=None):
    """models/tensorBase.py:565-589 -> (alpha [G0,G1,G2,T], dense_xyz [G0,G1,G2,3]); one native call per slab of G0"""
    gs, times, dense_xyz, slabs = _dense_lattice(field, gridSize, times)
    T = times.numel()
    alpha = torch.empty(gs[0], gs[1], gs[2], T, device=times.device)
    for i0, i1 in slabs:
        alpha_volume(field, dense_xyz[i0:i1].reshape(-1, 3), times, field._step_host, field.alphaMask,
                     out=alpha[i0:i1].view(-1, T))
    return alpha, dense_xyz


# ---- whole-scene volumes: both fields composed as the renderer composes a sample (csrc/rdrf_scene_alpha.hip) ----------------
SCENE_OUTPUTS = ("alpha", "owner", "sigma_s", "sigma_d", "blending")
SCENE_MAX_ENTRIES = (1 << 31) - 1   # include/rodynrf.h rdrf_scene_alpha: M * T of one call


def check_scene_fields(tensorf_static, tensorf, who):
    """the static field first, the dynamic field second, both on one device"""
    if getattr(tensorf_static, "DYNAMIC", None) is not False:
        raise L.RdrfError(f"{who}: tensorf_static must be the static field (TensorVMSplit)")
    if getattr(tensorf, "DYNAMIC", None) is not True:
        raise L.RdrfError(f"{who}: tensorf must be the dynamic field (TensorVMSplit_TimeEmbedding)")
    ds, dd = tensorf_static.aabb.device, tensorf.aabb.device
    if ds != dd:
        raise L.RdrfError(f"{who}: tensorf_static is on {ds} and tensorf on {dd}: both fields must be on one device")


@torch.no_grad()
def scene_alpha_volume(tensorf_static, tensorf, xyz, times, length=None, masks="fields", want=("alpha",), _out=None):
    """rdrf_scene_alpha: xyz [M,3] un-normalised, times [T] -> a dict of [M,T] tensors, one per name in `want` out of
    SCENE_OUTPUTS.  With a_f = 1 - exp(-sigma_f length) and the dynamic field's blending b:
    alpha = 1 - (1 - a_d b)(1 - a_s (1 - b)), what the compositor takes from the light at a sample of that length;
    owner = a_d b / (a_d b + a_s (1 - b)), the dynamic field's share (0 where both are empty).
    length: the sample length, by default the dynamic field's step (what getDenseAlpha uses).  masks: "fields" (each field's
    alphaMask), None, or (mask_s, mask_d), each an AlphaGridMask or None: a field is empty where its mask is."""
    who = "scene_alpha_volume"
    want = (want,) if isinstance(want, str) else tuple(want)
    bad = [w for w in want if w not in SCENE_OUTPUTS]
    if bad or not want:
        raise L.RdrfError(f"{who}: want = {want!r} must be a non-empty subset of {SCENE_OUTPUTS}")
    check_scene_fields(tensorf_static, tensorf, who)
    if isinstance(masks, str) and masks == "fields":
        masks = (tensorf_static.alphaMask, tensorf.alphaMask)
    elif masks is None:
        masks = (None, None)
    elif not isinstance(masks, (tuple, list)) or len(masks) != 2 or not all(m is None or isinstance(m, AlphaGridMask) for m in masks):
        raise L.RdrfError(f"{who}: masks must be \"fields\", None or (mask_s, mask_d) of AlphaGridMask / None, not {masks!r}")
    if not torch.is_tensor(xyz) or xyz.dim() < 1 or xyz.shape[-1] != 3:
        raise L.RdrfError(f"{who}: xyz must be a tensor [..., 3]")
    L.require_device(xyz)
    xyz = L.f32c(xyz.detach()).reshape(-1, 3)
    dev = xyz.device
    if dev != tensorf.aabb.device:
        raise L.RdrfError(f"{who}: xyz is on {dev} and the fields on {tensorf.aabb.device}")
    times = L.f32c(torch.as_tensor(times, dtype=torch.float32).detach().reshape(-1).to(dev))
    M, T = xyz.shape[0], times.numel()
    if T < 1:
        raise L.RdrfError(f"{who}: times is empty")
    length = float(tensorf._step_host if length is None else length)
    out = {w: torch.empty(M, T, device=dev) for w in want} if _out is None else _out
    if M == 0:
        return out
    PS, cs = field_structs(tensorf_static, tensorf_static._param_list(), "ndc")
    PD, cd = field_structs(tensorf, tensorf._param_list(), "ndc")
    ms, md = (None if m is None else m._struct() for m in masks)
    chunk = min(M, SCENE_MAX_ENTRIES // T)
    ws = L.workspace(dev, L.lib.rdrf_scene_alpha_ws_bytes(chunk, T))
    for a in range(0, M, chunk):
        b = min(M, a + chunk)
        o = [L.ptr(out[w][a:b]) if w in out else None for w in SCENE_OUTPUTS]
        L.check(L.lib.rdrf_scene_alpha(C.byref(PS), C.byref(cs), C.byref(PD), C.byref(cd), L.ptr(xyz[a:b]), b - a, L.ptr(times), T,
                                       length, None if ms is None else C.byref(ms), None if md is None else C.byref(md), *o,
                                       L.ptr(ws), ws.numel(), L.stream_of(xyz)), "rdrf_scene_alpha")
    return out


@torch.no_grad()
def scene_dense_alpha(tensorf_static, tensorf, gridSize=None, times=None, want_owner=False):
    """getDenseAlpha of the whole scene -> (alpha [G0,G1,G2,T][, owner [G0,G1,G2,T]], dense_xyz [G0,G1,G2,3]): the lattice
    of get_dense_alpha over the DYNAMIC field's aabb (its gridSize and lattice times by default), scene_alpha_volume with
    each field's alphaMask and the dynamic field's step per slab."""
    check_scene_fields(tensorf_static, tensorf, "scene_dense_alpha")
    gs, times, dense_xyz, slabs = _dense_lattice(tensorf, gridSize, times)
    T = times.numel()
    vols = {w: torch.empty(gs[0], gs[1], gs[2], T, device=times.device) for w in (("alpha", "owner") if want_owner else ("alpha",))}
    for i0, i1 in slabs:
        scene_alpha_volume(tensorf_static, tensorf, dense_xyz[i0:i1].reshape(-1, 3), times, want=tuple(vols),
                           _out={w: v[i0:i1].view(-1, T) for w, v in vols.items()})
    return tuple(vols.values()) + (dense_xyz,)


def build_mask(alpha, thres):
    """rdrf_alpha_mask_build: alpha [G0,G1,G2,T] -> (packed bits, stats int64[7] on the device)"""
    L.require_device(alpha)
    alpha = L.f32c(alpha)
    G0, G1, G2, T = alpha.shape
    bits = torch.empty((G0 * G1 * G2 * T + 7) // 8, dtype=torch.uint8, device=alpha.device)
    stats = torch.empty(7, dtype=torch.int64, device=alpha.device)
    L.check(L.lib.rdrf_alpha_mask_build(L.ptr(alpha), G0, G1, G2, T, float(thres), L.ptr(bits), L.ptr(stats),
                                        L.stream_of(alpha)), "rdrf_alpha_mask_build")
    return bits, stats


@torch.no_grad()
def update_alpha_mask(field, gridSize=(200, 200, 200)):
    """models/tensorBase.py:592-629: sets field.alphaMask, returns new_aabb (informational: shrink is not built)"""
    gs = [int(v) for v in gridSize]
    alpha, dense_xyz = get_dense_alpha(field, gs)
    bits, stats = build_mask(alpha, field.alphaMask_thres)
    st = stats.cpu().tolist()   # the one host transfer: count and box
    if st[0] == 0:
        raise L.RdrfError(f"updateAlphaMask: no lattice point of {gs} reaches alphaMask_thres = {field.alphaMask_thres}")
    T = alpha.shape[3]
    field.alphaMask = AlphaGridMask.from_packed(field.device, field.aabb, bits, (gs[2], gs[1], gs[0]), T)
    new_aabb = torch.stack((dense_xyz[st[1], st[2], st[3]], dense_xyz[st[4], st[5], st[6]]))
    field.alphaMask_stats = {"occupied": st[0], "total": gs[0] * gs[1] * gs[2] * T}
    return new_aabb


@torch.no_grad()
def filtering_rays(field, all_rays, all_rgbs, all_ts=None, N_samples=256, chunk=10240 * 5, bbox_only=False):
    """models/tensorBase.py:632-676.  bbox_only: the slab test against the field's aabb (torch).  Otherwise a ray is kept
    when any of its N_samples world-space samples lies in an occupied cell of field.alphaMask at the ray's time
    (all_ts [N]; without times, at any time).  Returns the kept (rays, rgbs) -- and the kept times when given."""
    N = int(np.prod(all_rays.shape[:-1]))
    rays_flat = all_rays.reshape(N, -1)
    ts_flat = None if all_ts is None else torch.as_tensor(all_ts).reshape(N)
    dev = field.aabb.device
    if not bbox_only and field.alphaMask is None:
        raise L.RdrfError("filtering_rays: the field has no alphaMask (updateAlphaMask) -- or pass bbox_only=True")
    kept = []
    for i0 in range(0, N, int(chunk)):
        rays = rays_flat[i0:i0 + int(chunk)].to(dev).float()
        rays_o, rays_d = rays[..., :3], rays[..., 3:6]
        if bbox_only:
            vec = torch.where(rays_d == 0, torch.full_like(rays_d, 1e-6), rays_d)
            rate_a = (field.aabb[1] - rays_o) / vec
            rate_b = (field.aabb[0] - rays_o) / vec
            t_min = torch.minimum(rate_a, rate_b).amax(-1)
            t_max = torch.maximum(rate_a, rate_b).amin(-1)
            inb = t_max > t_min
        else:
            xyz, _, _ = field.sample_ray(rays_o, rays_d, is_train=False, N_samples=N_samples)
            n, S = xyz.shape[:2]
            if ts_flat is not None:
                tlist = [ts_flat[i0:i0 + int(chunk)].to(dev).float()]
            else:
                tlist = [torch.full((n,), float(v), device=dev) for v in lattice_times(max(field.alphaMask.tSize, 2))]
            inb = torch.zeros(n, dtype=torch.bool, device=dev)
            for tt in tlist:
                inb |= apply_alpha_mask(torch.ones(n, S, dtype=torch.bool, device=dev), xyz, tt, field.alphaMask).any(-1)
        kept.append(inb.to(all_rays.device))
    mask = torch.cat(kept).view(all_rgbs.shape[:-1])
    out = (all_rays[mask], all_rgbs[mask])
    return out if all_ts is None else out + (torch.as_tensor(all_ts)[mask],)


def mask_to_ckpt(mask):
    """the three checkpoint entries of models/tensorBase.py:465-469"""
    return {"alphaMask.shape": mask.shape, "alphaMask.mask": mask.packed.cpu().numpy(), "alphaMask.aabb": mask.aabb.cpu()}


def mask_from_ckpt(ckpt, device, tSize=None):
    """models/tensorBase.py:473-484, with the tSize the reference forgets to pass (the last entry of the stored shape)"""
    shape = tuple(int(v) for v in ckpt["alphaMask.shape"])
    T = shape[-1] if tSize is None else int(tSize)
    if shape[-1] != T:
        raise L.RdrfError(f"checkpoint alphaMask has {shape[-1]} time slices, the field has tSize {T}")
    return AlphaGridMask.from_packed(device, ckpt["alphaMask.aabb"], ckpt["alphaMask.mask"], shape[-4:-1], T)
