"""Host mirror of /root/reference/renderer.py:24-315 for the hot path: ``sampleXYZ``,
``raw2outputs`` and a working ``OctreeRender_trilinear_fast`` chunk loop.  All arithmetic runs in
the HIP kernels (rdrf_sample_*, rdrf_composite_*); torch only supplies memory, RNG and autograd."""
import ctypes as C
from collections import namedtuple

import torch

from . import _lib as L
from ._params import field_structs, render_structs

# the per-ray outputs of raw2outputs (renderer.py:173-315) that the eval loop keeps per frame (renderer.py:745-826):
# rgb / depth / acc of the full, static (_s) and dynamic (_d) renders and the blending ("dynamicness") map
RenderMaps = namedtuple("RenderMaps", L.RENDER_MAPS)
# the thirteen per-ray outputs of raw2outputs in the reference's order (renderer.py:301-315): colour [N,3], depth [N], acc [N]
# and sample weights [N,S] of the full, the static (_s) and the dynamic (_d) render, then the blending map
RayMaps = namedtuple("RayMaps", ("rgb", "depth", "acc", "weights", "rgb_s", "depth_s", "acc_s", "weights_s", "rgb_d", "depth_d",
                                 "acc_d", "weights_d", "dynamicness"))
# the motion maps of the per-frame render (renderer.py:487-537, :610): induced optical flow to the next / previous frame
# through the scene-flow MLP (flow_f, flow_b) and through camera motion alone (flow_s_f, flow_s_b), [N,2] pixels, and the
# warp displacement sum_s weights_d (xyz_prime - xyz) [N,3]
MotionMaps = namedtuple("MotionMaps", L.MOTION_MAPS)
# point tracks (track_points): points [M,K,3] in field coordinates, pixels [M,K,2] and disp [M,K] in camera k (None without
# cameras), frames_offset [K] = -n_bwd .. n_fwd: slot k is the seed's frame + frames_offset[k]
Tracks = namedtuple("Tracks", ("points", "pixels", "disp", "frames_offset"))


class _SampleFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rays, aabb_host, near, far, S, ray_type, jitter, jitter_outer, step):
        ctx.set_materialize_grads(False)
        L.require_device(rays)
        rays = L.f32c(rays)
        N = rays.shape[0]
        dev = rays.device
        xyz = torch.empty(N, S, 3, device=dev)
        z = torch.empty(N, S, device=dev)
        valid = torch.empty(N, S, dtype=torch.uint8, device=dev)
        if ray_type == "ndc":
            ab = (C.c_float * 6)(*aabb_host)
            L.check(L.lib.rdrf_sample_ndc(L.ptr(rays), N, S, near, far,
                                          L.ptr(jitter), ab, L.ptr(xyz), L.ptr(z), L.ptr(valid),
                                          L.stream_of(rays)), "rdrf_sample_ndc")
        elif ray_type == "contract":
            L.check(L.lib.rdrf_sample_contract(L.ptr(rays), N, S, near, far,
                                               L.ptr(jitter), L.ptr(jitter_outer), L.ptr(xyz),
                                               L.ptr(z), L.ptr(valid), L.stream_of(rays)),
                    "rdrf_sample_contract")
        else:   # every other ray_type marches in world space (models/tensorBase.py:501-522); jitter: one value per ray
            ab = (C.c_float * 6)(*aabb_host)
            L.check(L.lib.rdrf_sample_world(L.ptr(rays), N, S, near, far, step,
                                            L.ptr(jitter), ab, L.ptr(xyz), L.ptr(z), L.ptr(valid),
                                            L.stream_of(rays)), "rdrf_sample_world")
            ctx.world = (ab, near, far)
        ctx.ray_type = ray_type
        ctx.save_for_backward(rays, z)
        if ray_type in L.RAY_TYPES:
            ctx.mark_non_differentiable(valid, z)
        else:   # these z depend on the ray (through the entry depth t_min)
            ctx.mark_non_differentiable(valid)
        return xyz, z, valid.view(torch.bool)

    @staticmethod
    def backward(ctx, g_xyz, g_z, g_valid):
        rays, z = ctx.saved_tensors
        N, S = z.shape
        none = (None,) * 9
        if ctx.ray_type not in L.RAY_TYPES:
            if g_xyz is None and g_z is None:
                return none
            g_rays = torch.zeros_like(rays)
            g_xyz = None if g_xyz is None else L.f32c(g_xyz)
            g_z = None if g_z is None else L.f32c(g_z)
            ab, near, far = ctx.world
            L.check(L.lib.rdrf_sample_world_bwd(L.ptr(rays), L.ptr(z), N, S, near, far, ab,
                                                L.ptr(g_xyz), L.ptr(g_z), L.ptr(g_rays), L.stream_of(rays)),
                    "rdrf_sample_world_bwd")
            return (g_rays,) + none[1:]
        if g_xyz is None:   # z_vals / valid carry no gradient to the rays
            return none
        g_rays = torch.zeros_like(rays)
        g_xyz = L.f32c(g_xyz)
        L.check(L.lib.rdrf_sample_bwd(L.ptr(rays), L.ptr(z), N, S, L.RAY_TYPES[ctx.ray_type],
                                      L.ptr(g_xyz), L.ptr(g_rays), L.stream_of(rays)),
                "rdrf_sample_bwd")
        return (g_rays,) + none[1:]


def sample_rays(tensorf, rays, N_samples, ray_type="ndc", is_train=False, jitter=None,
                jitter_outer=None):
    """sample_ray_ndc / sample_ray_contracted with the z row tiled to [N,S]
    (models/tensorBase.py:487-559 + renderer.py:169). The train-time jitter is drawn with torch's
    device RNG here unless given.
    Any other ray_type -- write "world" -- is sample_ray (models/tensorBase.py:501-522): the rays march through the
    field's aabb in world space, tensorf.stepSize apart, from their entry depth clamped to near_far; z_vals [N,S] are
    per ray as sample_ray returns them, and `jitter` is ONE value per ray, [N]."""
    near, far = tensorf.near_far
    S = int(N_samples)
    dev = rays.device
    if ray_type not in L.RAY_TYPES:
        N = rays.shape[0]
        if is_train and jitter is None:
            jitter = torch.rand(N, device=dev)
        if jitter is not None:
            jitter = L.f32c(jitter.reshape(-1))
            if jitter.numel() != N:
                raise L.RdrfError(f"sample_rays: the world-space march takes one jitter value per ray ({N}), got {jitter.numel()}")
        return _SampleFn.apply(rays, tensorf._aabb_host, float(near), float(far), S, ray_type, jitter, None,
                               tensorf._step_host)
    if is_train and jitter is None:
        if ray_type == "ndc":
            jitter = torch.rand(S, device=dev)
        else:
            jitter = torch.rand(S - S // 2 + 1, device=dev)
            jitter_outer = torch.rand(S // 2 + 1, device=dev)
    if jitter is not None:
        jitter = L.f32c(jitter.reshape(-1))
    if jitter_outer is not None:
        jitter_outer = L.f32c(jitter_outer.reshape(-1))
    return _SampleFn.apply(rays, tensorf._aabb_host, float(near), float(far), S, ray_type, jitter,
                           jitter_outer, None)


def sampleXYZ(tensorf, rays_train, N_samples, ray_type="ndc", is_train=False, jitter=None,
              jitter_outer=None):
    """renderer.py:147-170 (extra keyword: explicit jitter vectors for reproducible tests).  ray_type "ndc", "contract" or
    "world" (any other string: the reference's `else` branch, TensorBase.sample_ray)."""
    if N_samples is None or N_samples <= 0:
        N_samples = tensorf.nSamples
    return sample_rays(tensorf, rays_train, N_samples, ray_type, is_train, jitter, jitter_outer)


class _CompositeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rgb_s, sigma_s, rgb_d, sigma_d, dists, blending, z_vals, rays, ray_type,
                add_white_bg):
        ctx.set_materialize_grads(False)
        L.require_device(rgb_s, sigma_s, rgb_d, sigma_d, dists, blending, z_vals, rays)
        ins = [L.f32c(t) for t in (rgb_s, sigma_s, rgb_d, sigma_d, dists, blending, z_vals, rays)]
        N, S = ins[1].shape
        dev = ins[1].device
        shapes = [(N, 3), (N,), (N,), (N, S)] * 3 + [(N,)]
        outs = [torch.empty(s, device=dev) for s in shapes]
        arr = (C.c_void_p * 13)(*[o.data_ptr() for o in outs])
        # the coin as a device float (one element, 0 / 1): read when the kernel runs, so a captured HIP graph of the
        # iteration follows each replay's coin (step.Trainer(graph=True)); a host bool otherwise
        white_dev = add_white_bg if torch.is_tensor(add_white_bg) else None
        if white_dev is not None and (white_dev.dtype != torch.float32 or white_dev.numel() != 1 or not white_dev.is_cuda):
            raise L.RdrfError("raw2outputs: a device coin is one fp32 element on the GPU")
        white = 0 if white_dev is not None else int(add_white_bg)
        L.check(L.lib.rdrf_composite_fwd(*[L.ptr(t) for t in ins], N, S, L.RAY_TYPES.get(ray_type, 2),
                                         white, L.ptr(white_dev), arr, L.stream_of(ins[1])),
                "rdrf_composite_fwd")
        ctx.ray_type, ctx.white, ctx.white_dev = ray_type, white, white_dev
        ctx.save_for_backward(*ins)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *g_out):
        ins = ctx.saved_tensors
        N, S = ins[1].shape
        g_out = [None if g is None else L.f32c(g) for g in g_out]
        need = list(ctx.needs_input_grad[:8])
        # like autograd on the reference's op graph, a branch no loss reaches gets NO gradient (not a
        # zero one): rgb_s only feeds rgb_map_full / rgb_map_s, rgb_d only rgb_map_full / rgb_map_d.
        # The field's backward then skips its whole appearance half (MLP, scatter, dW) for that pass.
        have = lambda idx: any(g_out[i] is not None for i in idx)
        need[0] = need[0] and have((0, 4))
        need[2] = need[2] and have((0, 8))
        # sigma_s feeds the full and the static maps, sigma_d / blending the full and the dynamic maps
        # (renderer.py:190-262): e.g. pass E of the trainer consumes only rgb_map_s / depth_map_s, so
        # the dynamic field gets no gradient at all from it
        need[1] = need[1] and have((0, 1, 2, 3, 4, 5, 6, 7, 12))
        need[3] = need[3] and have((0, 1, 2, 3, 8, 9, 10, 11, 12))
        # blending only enters T_full / weights_full (renderer.py:206-262): the dynamic-only maps (8..11) do not depend
        # on it, so a loss on depth_map_d / weights_d alone (passes B-D of the trainer) sends the blending head NO
        # gradient -- and the field's backward then leaves that head, its scatter set and its dW products out
        need[5] = need[5] and have((0, 1, 2, 3, 12))
        # z_vals only enters the three depth maps (renderer.py:283-285), the rays only their NDC far-plane term
        # (renderer.py:287-291): without a depth cotangent -- or, for the rays, outside NDC -- autograd gives them NO gradient
        need[6] = need[6] and have((1, 5, 9))
        need[7] = need[7] and ctx.ray_type == "ndc" and have((1, 5, 9))
        g_in = L.zeros_like_many(ins, need)   # one fill for the (up to eight) gradient tensors
        ga = (C.c_void_p * 13)(*[0 if g is None else g.data_ptr() for g in g_out])
        gi = (C.c_void_p * 8)(*[0 if g is None else g.data_ptr() for g in g_in])
        L.check(L.lib.rdrf_composite_bwd(*[L.ptr(t) for t in ins], N, S,
                                         L.RAY_TYPES.get(ctx.ray_type, 2), ctx.white, L.ptr(ctx.white_dev), ga, gi,
                                         L.stream_of(ins[1])), "rdrf_composite_bwd")
        return (*g_in, None, None)


def raw2outputs(rgb_s, sigma_s, rgb_d, sigma_d, dists, blending, z_vals, rays_chunk, is_train=False,
                ray_type="ndc", add_white_bg=None):
    """renderer.py:173-315.  The train-time coin (`torch.rand((1,)) < 0.5`, renderer.py:269) is
    drawn here on the host unless `add_white_bg` is given: a bool, or a one-element fp32 DEVICE tensor (0 / 1) that the
    kernels read when they run."""
    if add_white_bg is None:
        add_white_bg = bool(is_train and (torch.rand((1,)) < 0.5).item())
    return RayMaps(*_CompositeFn.apply(rgb_s, sigma_s, rgb_d, sigma_d, dists, blending, z_vals, rays_chunk,
                                       ray_type, add_white_bg if torch.is_tensor(add_white_bg) else bool(add_white_bg)))


def OctreeRender_trilinear_fast(rays, ts, timeembeddings, tensorf, xyz_sampled, z_vals_input,
                                ray_valid, chunk=4096, N_samples=-1, ray_type="ndc", white_bg=True,
                                is_train=False, device="cuda"):
    """renderer.py:24-144 -- same signature and 11-tuple; unlike the reference (which raises on
    its own None entries) this chunk loop tolerates them."""
    keys = [[] for _ in range(10)]
    N = rays.shape[0]
    for c0 in range(0, N, chunk):
        sl = slice(c0, c0 + chunk)
        te = None if timeembeddings is None else timeembeddings[sl].to(device)
        out = tensorf(rays[sl].to(device), ts[sl].to(device), te, xyz_sampled[sl].to(device),
                      z_vals_input[sl].to(device), ray_valid[sl].to(device), is_train=is_train,
                      white_bg=white_bg, ray_type=ray_type, N_samples=N_samples)
        out = list(out)
        if out[5] is not None:
            out[5] = out[5] - xyz_sampled[sl].to(device)  # delta_xyz
        for k, v in zip(keys, out):
            k.append(v)
    cat = lambda l: None if any(v is None for v in l) else torch.cat(l)
    r = [cat(k) for k in keys]
    return (r[0], r[1], r[2], r[3], r[4], r[5], None, r[6], r[7], r[8], r[9])


def _map_names(maps):
    """maps=True: all ten; else an iterable of RenderMaps field names (the others are not written)"""
    names = L.RENDER_MAPS if maps is True else tuple(maps)
    bad = [n for n in names if n not in L.RENDER_MAPS]
    if bad or not names:
        raise ValueError(f"maps: True or a non-empty subset of {L.RENDER_MAPS}, got {maps!r}")
    return names


def _alloc_maps(names, N, dev):
    return {n: torch.empty((N, 3) if n.startswith("rgb") else (N,), device=dev) for n in names}


def _maps_struct(bufs):
    return L.RenderMapsC(*[bufs[n].data_ptr() if n in bufs else None for n in L.RENDER_MAPS])


def _map_outputs(maps, N, dev):
    """the output buffers of a render by name -- the requested `maps`, else rgb and depth -- and the RdrfRenderMaps of them"""
    bufs = _alloc_maps(_map_names(maps) if maps else ("rgb", "depth"), N, dev)
    return bufs, _maps_struct(bufs)


def _map_result(bufs, maps):
    """what a render returns of _map_outputs' buffers: a RenderMaps with `maps`, else (rgb, depth)"""
    return RenderMaps(**{n: bufs.get(n) for n in L.RENDER_MAPS}) if maps else (bufs["rgb"], bufs["depth"])


def _motion_names(want):
    """True: all five; else an iterable of MotionMaps field names (the others are not computed)"""
    names = L.MOTION_MAPS if want is True else tuple(want)
    bad = [n for n in names if n not in L.MOTION_MAPS]
    if bad or not names:
        raise ValueError(f"motion maps: True or a non-empty subset of {L.MOTION_MAPS}, got {want!r}")
    return names


def _motion_request(motion, N, dev):
    """motion: dict of H, W, focal, c2w_f, c2w_b [3,4], first_pixel (default 0) and maps (default True: all five).
    Returns (output buffers by name, RdrfMotionMaps, RdrfMotionCams, tensors the structs point into)."""
    names = _motion_names(motion.get("maps", True))
    bufs = {n: torch.empty((N, 3) if n == "delta_xyz" else (N, 2), device=dev) for n in names}
    focal = motion["focal"]
    focal = _focal_tensor(focal.to(dev) if torch.is_tensor(focal) else focal, dev).contiguous()
    pose = [L.f32c(torch.as_tensor(motion[k], dtype=torch.float32).detach().to(dev)) for k in ("c2w_f", "c2w_b")]
    if any(p_.shape != (3, 4) for p_ in pose):
        raise L.RdrfError("motion: c2w_f and c2w_b are [3,4] camera-to-world matrices")
    cams = L.MotionCamsC(int(motion["H"]), int(motion["W"]), focal.data_ptr(), pose[0].data_ptr(), pose[1].data_ptr(),
                         int(motion.get("first_pixel", 0)))
    mm = L.MotionMapsC(*[bufs[n].data_ptr() if n in bufs else None for n in L.MOTION_MAPS])
    return bufs, mm, cams, (focal, pose)


def _mask_pair(tensorf_static, tensorf, alpha_masks):
    """alpha_masks of render_rays -> None (no masks) or the pair (static, dynamic), at least one of them a mask"""
    if alpha_masks is None or alpha_masks is False:
        return None
    if alpha_masks is True:
        alpha_masks = (tensorf_static.alphaMask, tensorf.alphaMask)
    pair = tuple(alpha_masks)
    if len(pair) != 2:
        raise ValueError("alpha_masks: True or a pair (mask_static, mask_dynamic)")
    if pair[0] is None and pair[1] is None:
        raise ValueError("alpha_masks: both masks are None (updateAlphaMask builds a field's mask)")
    return pair


def _n_samples(tensorf, N_samples):
    """samples per ray of a render: the caller's count, or the dynamic field's"""
    return int(N_samples) if N_samples and N_samples > 0 else tensorf.nSamples


@torch.no_grad()
def render_rays(tensorf_static, tensorf, rays, ts, N_samples=-1, ray_type="ndc", mode="auto", maps=False, motion=None,
                alpha_masks=None, kept=None):
    """No-grad render of a ray chunk through ONE C-ABI call: the loop body of renderer.py:740-812.
    mode "auto" (rdrf_render_fwd: the per-phase launch sequence), "fused" (rdrf_render_fused_fwd:
    one cooperative launch) or "sequence" (rdrf_render_sequence_fwd); all three give the same bits.
    ray_type "ndc", "contract" or "world" (any other string: the world-space march of sample_rays, through
    rdrf_render_world_fwd; no `motion` for it).
    Returns (rgb_map_full[N,3], depth_map_full[N]); with `maps` (True, or a subset of the RenderMaps field names)
    a RenderMaps of the per-ray outputs ([N,3] rgb maps, [N] others; None where not requested), through
    rdrf_render_maps_fwd: the same bits as raw2outputs after the fields' forward.
    With `motion` (a dict: H, W, focal, c2w_f, c2w_b -- the [3,4] poses of the next / previous frame --, first_pixel = flat
    pixel of ray 0 in the H x W image (default 0), maps = True or a subset of the MotionMaps field names) the call goes
    through rdrf_render_motion_fwd and returns (the above, MotionMaps): the induced-flow and warp-displacement maps of
    renderer.py:487-537, :610 from the render's own workspace, the colour maps bit for bit as without `motion`.
    With `alpha_masks` -- a pair (mask_static, mask_dynamic) of AlphaGridMask or None, or True for
    (tensorf_static.alphaMask, tensorf.alphaMask) -- the call goes through rdrf_render_masked_fwd: the maps are those of
    apply_alpha_mask on the sampler's `valid` per field, the fields' forward and raw2outputs, bit for bit, and the density
    phase of a field runs on the samples its mask keeps only.  `kept`: an int64 device tensor [2] that receives the kept
    sample counts (static, dynamic).  No mode "fused" and no `motion` with masks."""
    masks = _mask_pair(tensorf_static, tensorf, alpha_masks)
    if masks is None and kept is not None:
        raise ValueError("render_rays: `kept` is the masked render's output (alpha_masks)")
    if masks is not None:
        if mode == "fused":
            raise NotImplementedError("render_rays: the single-launch render (mode='fused') reads no alpha masks.")
        if motion is not None:
            raise NotImplementedError("render_rays: no motion maps with alpha masks (xyz_prime of a dropped sample is undefined).")
    L.require_device(rays, ts)
    rays, ts = L.f32c(rays), L.f32c(ts)
    N = rays.shape[0]
    S = _n_samples(tensorf, N_samples)
    dev = rays.device
    ws = L.workspace(dev, (L.lib.rdrf_render_motion_workspace_bytes if motion is not None else L.lib.rdrf_render_workspace_bytes)(N, S))
    PS, cs, PD, cd = render_structs(tensorf_static, tensorf, ray_type)
    head = (C.byref(PS), C.byref(cs), C.byref(PD), C.byref(cd), L.ptr(rays), L.ptr(ts), N, S)
    near, far = tensorf.near_far
    bufs, M = _map_outputs(maps, N, dev)
    if masks is not None:
        if kept is not None and (kept.dtype != torch.int64 or kept.numel() != 2 or not kept.is_cuda or not kept.is_contiguous()):
            raise L.RdrfError("render_rays: `kept` is a contiguous int64 device tensor of two elements")
        ms, md = (None if m is None else m._struct() for m in masks)
        ws = L.workspace(dev, L.lib.rdrf_render_masked_ws_bytes(N, S))
        step = 0.0 if ray_type in L.RAY_TYPES else tensorf._step_host
        L.check(L.lib.rdrf_render_masked_fwd(*head, near, far, step, None if ms is None else C.byref(ms),
                                             None if md is None else C.byref(md), C.byref(M), L.ptr(kept), L.ptr(ws),
                                             ws.numel(), L.stream_of(rays)), "rdrf_render_masked_fwd")
        return _map_result(bufs, maps)
    if motion is not None:
        if ray_type not in L.RAY_TYPES:
            raise NotImplementedError("motion maps: ray_type must be 'ndc' or 'contract' (the reference projects no other, "
                                      "renderer.py:1335-1351)")
        mbufs, MM, cams, keep = _motion_request(motion, N, dev)
        L.check(L.lib.rdrf_render_motion_fwd(*head, near, far, L.RENDER_MODES[mode], C.byref(M), C.byref(cams), C.byref(MM),
                                             L.ptr(ws), ws.numel(), L.stream_of(rays)), "rdrf_render_motion_fwd")
        del keep
        return _map_result(bufs, maps), MotionMaps(**{n: mbufs.get(n) for n in L.MOTION_MAPS})
    if ray_type not in L.RAY_TYPES:   # world-space rays: one entry point for the family, it carries the sampler's step
        L.check(L.lib.rdrf_render_world_fwd(*head, 0, near, far, tensorf._step_host, L.RENDER_MODES[mode], C.byref(M), L.ptr(ws),
                                            ws.numel(), L.stream_of(rays), None, 0), "rdrf_render_world_fwd")
        return _map_result(bufs, maps)
    if maps:
        L.check(L.lib.rdrf_render_maps_fwd(*head, near, far, L.RENDER_MODES[mode], C.byref(M), L.ptr(ws), ws.numel(),
                                           L.stream_of(rays)), "rdrf_render_maps_fwd")
    else:
        fn = {"auto": L.lib.rdrf_render_fwd, "fused": L.lib.rdrf_render_fused_fwd, "sequence": L.lib.rdrf_render_sequence_fwd}[mode]
        L.check(fn(*head, near, far, L.ptr(bufs["rgb"]), L.ptr(bufs["depth"]), L.ptr(ws), ws.numel(), L.stream_of(rays)),
                "rdrf_render_" + mode)
    return _map_result(bufs, maps)


_stream_pool = {}


@torch.no_grad()
def render_chunks(tensorf_static, tensorf, rays, ts, chunk, N_samples=-1, ray_type="ndc", streams=8, maps=False,
                  alpha_masks=None):
    """The chunk loop of renderer.py:740-812 (`for chunk_idx in range(N_rays_all // chunk + ...)`, chunk = 512 at
    renderer.py:732) as ONE native call (rdrf_render_chunks_fwd): the chunks' launch sequences are issued from C,
    round-robin on `streams` HIP streams (0 / 1: all on the current stream).  Issued chunk by chunk from Python the loop
    is host-bound (~250 us of marshalling per chunk against ~190 us of GPU work); and one 512-ray chunk fills only
    64-110 of the 256 CUs, so independent chunks run side by side.  Same bits as render_rays on the whole batch.
    Returns (rgb_map [N,3], depth_map [N]); with `maps`, a RenderMaps as render_rays (rdrf_render_chunks_maps_fwd).
    `alpha_masks` is not built here (render_rays has it)."""
    if alpha_masks is not None and alpha_masks is not False:
        raise NotImplementedError("render_chunks: the native chunk loop reads no alpha masks (render_rays does).")
    L.require_device(rays, ts)
    rays, ts = L.f32c(rays), L.f32c(ts)
    N, dev = rays.shape[0], rays.device
    S = _n_samples(tensorf, N_samples)
    chunk = int(chunk)
    bufs, M = _map_outputs(maps, N, dev)
    if N == 0:
        return _map_result(bufs, maps)
    ns = int(streams) if streams and streams > 1 and N > chunk else 0
    ws = L.workspace(dev, L.lib.rdrf_render_chunks_workspace_bytes(min(chunk, N), S, max(ns, 1)))
    # one packed image per field, packed on the current stream, shared read-only by every side stream
    PS, cs, PD, cd = render_structs(tensorf_static, tensorf, ray_type)
    head = (C.byref(PS), C.byref(cs), C.byref(PD), C.byref(cd), L.ptr(rays), L.ptr(ts), N, S)
    near, far = tensorf.near_far
    pool = _stream_pool.get((dev, ns))
    if pool is None:
        pool = _stream_pool[(dev, ns)] = [torch.cuda.Stream(device=dev) for _ in range(ns)]
    arr = (C.c_void_p * max(ns, 1))(*[st.cuda_stream for st in pool]) if ns else None
    if ray_type not in L.RAY_TYPES:   # world-space rays (see render_rays)
        L.check(L.lib.rdrf_render_world_fwd(*head, chunk, near, far, tensorf._step_host, 0, C.byref(M), L.ptr(ws), ws.numel(),
                                            L.stream_of(rays), arr, ns), "rdrf_render_world_fwd")
    elif maps:
        L.check(L.lib.rdrf_render_chunks_maps_fwd(*head, chunk, near, far, C.byref(M), L.ptr(ws), ws.numel(), L.stream_of(rays),
                                                  arr, ns), "rdrf_render_chunks_maps_fwd")
    else:
        L.check(L.lib.rdrf_render_chunks_fwd(*head, chunk, near, far, L.ptr(bufs["rgb"]), L.ptr(bufs["depth"]), L.ptr(ws),
                                             ws.numel(), L.stream_of(rays), arr, ns), "rdrf_render_chunks_fwd")
    for st in pool:   # the caching allocator must not hand these buffers to another stream's request while the side
        for t in [rays, ts, ws, *bufs.values()]:   # streams may still read / write them
            t.record_stream(st)
    return _map_result(bufs, maps)


def _render_image(tensorf_static, tensorf, rays, ts, H, W, N_samples, ray_type, chunk, maps, motion=None, alpha_masks=None):
    """the rays of one H x W image through render_rays in chunks (default: the whole image in one launch sequence);
    `motion`: the dict of render_rays without first_pixel (every chunk passes its own) -> (images, MotionMaps of images);
    `alpha_masks`: as render_rays"""
    dev = rays.device
    S_ = _n_samples(tensorf, N_samples)
    if not chunk:   # whole frame in one launch sequence, bounded by the kernels' 32-bit sample indices
        chunk = max(1, min(H * W, (2 ** 31 - 1) // (3 * S_) - 1))
    chunk = int(chunk)
    mout = None
    if motion is not None:
        mnames = _motion_names(motion.get("maps", True))
        mout = {n: torch.empty((H * W, 3) if n == "delta_xyz" else (H * W, 2), device=dev) for n in mnames}

    def run(c0, want):
        if motion is None:
            return render_rays(tensorf_static, tensorf, rays[c0:c0 + chunk], ts[c0:c0 + chunk], N_samples, ray_type, maps=want,
                               alpha_masks=alpha_masks)
        part, mpart = render_rays(tensorf_static, tensorf, rays[c0:c0 + chunk], ts[c0:c0 + chunk], N_samples, ray_type,
                                  maps=want, motion=dict(motion, first_pixel=c0), alpha_masks=alpha_masks)
        for n in mout:
            mout[n][c0:c0 + chunk] = getattr(mpart, n)
        return part

    def finish(images):
        if motion is None:
            return images
        return images, MotionMaps(**{n: None if n not in mout else mout[n].view(H, W, -1) for n in L.MOTION_MAPS})

    if not maps:
        rgb = torch.empty(H * W, 3, device=dev)
        depth = torch.empty(H * W, device=dev)
        for c0 in range(0, H * W, chunk):
            r, d = run(c0, False)
            rgb[c0:c0 + chunk], depth[c0:c0 + chunk] = r, d
        return finish((rgb.clamp_(0.0, 1.0).view(H, W, 3), depth.view(H, W)))
    names = _map_names(maps)
    if chunk >= H * W:
        out = run(0, names)._asdict()
    else:
        out = _alloc_maps(names, H * W, dev)
        for c0 in range(0, H * W, chunk):
            part = run(c0, names)
            for n in names:
                out[n][c0:c0 + chunk] = getattr(part, n)
    for n in ("rgb", "rgb_s", "rgb_d", "blending"):   # renderer.py:829-832; the depths stay raw
        if out.get(n) is not None:
            out[n].clamp_(0.0, 1.0)
    return finish(RenderMaps(**{n: None if out.get(n) is None else out[n].view(H, W, 3) if n.startswith("rgb") else out[n].view(H, W)
                                for n in L.RENDER_MAPS}))


@torch.no_grad()
def render_frame(tensorf_static, tensorf, poses9, focal, frame, H, W, N_samples=-1, ray_type="ndc",
                 chunk=None, t=None, maps=False, motion=False, alpha_masks=None):
    """Whole-frame no-grad render (the per-image body of renderer.py:661-966 `evaluation`): rays of
    every pixel of `frame` are generated on the device and pushed through rdrf_render_fwd in chunks
    (default: the whole frame in one launch sequence).  `t` overrides the frame's own time in [-1,1].
    Returns (rgb [H,W,3] clamped to [0,1], depth [H,W]).  With `maps` (True, or a subset of the RenderMaps field names):
    a RenderMaps of [H,W,3] / [H,W] images, rgb, rgb_s, rgb_d and blending clamped to [0,1] as renderer.py:829-832, the
    depths raw.  (For contract scenes the reference writes the depths as -1 / (d + 1e-6), renderer.py:862-865: that display
    transform is the caller's.)
    With `motion` (True, or a subset of the MotionMaps field names): returns (the above, MotionMaps) with the flows as
    [H,W,2] and delta_xyz as [H,W,3]; the neighbour cameras are the reference's, frames min(frame + 1, T - 1) and
    max(frame - 1, 0) of `poses9` (renderer.py:386-387).
    `alpha_masks`: as render_rays (the masked render; not together with `motion`)."""
    from .ray_utils import generate_rays, pose_to_mtx
    dev = poses9.device
    T = poses9.shape[0]
    ids = torch.arange(H * W, device=dev) + int(frame) * H * W
    rays = generate_rays(ids, poses9, focal, H, W, ndc=ray_type == "ndc", near=1.0)
    tv = (2.0 * frame / max(T - 1, 1) - 1.0) if t is None else float(t)
    ts = torch.full((H * W,), tv, device=dev)
    req = None
    if motion:
        mtx = pose_to_mtx(poses9.detach().float())
        req = dict(H=H, W=W, focal=focal, c2w_f=mtx[min(int(frame) + 1, T - 1)], c2w_b=mtx[max(int(frame) - 1, 0)], maps=motion)
    return _render_image(tensorf_static, tensorf, rays, ts, H, W, N_samples, ray_type, chunk, maps, req, alpha_masks)


def _focal_per_camera(focal, B, dev):
    f = torch.as_tensor(focal, dtype=torch.float32, device=dev).reshape(-1)
    if f.numel() == 1:
        return f.expand(B).contiguous()
    if f.numel() != B:
        raise L.RdrfError(f"camera_rays: focal must be a scalar or one value per camera ({B}), got {f.numel()}")
    return f.contiguous()


def camera_rays(c2w, focal, H, W, ndc=True, near=1.0, first=0, n=None):
    """Rays [n,6] of the flat pixels first .. first + n - 1 over (B, H, W) of the cameras c2w [B,3,4] (or [3,4]), focal a
    scalar or one per camera: get_ray_directions_blender -> get_rays -> ndc_rays_blender (with `near`) when `ndc`
    (dataLoader/ray_utils.py:93-110, 143-160, 197-218; the eval rays of renderer.py:702-716, 1013-1030) in one kernel
    (rdrf_camera_rays).  World rays keep unnormalised directions, as get_rays does.  No gradient (eval is no-grad)."""
    L.require_device(c2w)
    dev = c2w.device
    c2w = L.f32c(c2w.detach().reshape(-1, 3, 4))
    B = c2w.shape[0]
    f = _focal_per_camera(focal.detach() if torch.is_tensor(focal) else focal, B, dev)
    n = B * int(H) * int(W) - int(first) if n is None else int(n)
    rays = torch.empty(n, 6, device=dev)
    L.check(L.lib.rdrf_camera_rays(L.ptr(c2w), L.ptr(f), B, int(H), int(W), int(bool(ndc)), float(near), int(first), n,
                                   L.ptr(rays), L.stream_of(c2w)), "rdrf_camera_rays")
    return rays


@torch.no_grad()
def render_view(tensorf_static, tensorf, c2w, focal, H, W, t, N_samples=-1, ray_type="ndc", maps=True, chunk=None,
                c2w_f=None, c2w_b=None, motion=False, alpha_masks=None):
    """One arbitrary camera c2w [3,4] (host or device; moved to the fields' device) at time t in [-1,1]: the per-view body
    of renderer.py:970-1263 `evaluation_path` (eval rays: camera_rays, NDC with near = 1 for ndc scenes; ray_type "world":
    the camera's un-normalised world rays marched through the aabb, see sample_rays).  Returns a
    RenderMaps of [H,W,3] / [H,W] images (clamped as render_frame) with `maps`, else (rgb [H,W,3], depth [H,W]).
    With `motion` (True, or a subset of the MotionMaps field names) and the neighbour cameras c2w_f / c2w_b [3,4] (default:
    the view's own camera): returns (the above, MotionMaps of [H,W,2] / [H,W,3] images) as render_frame.
    `alpha_masks`: as render_rays (the masked render; not together with `motion`)."""
    if motion and ray_type not in L.RAY_TYPES:
        raise NotImplementedError("motion maps: ray_type must be 'ndc' or 'contract' (the reference projects no other, "
                                  "renderer.py:1335-1351)")
    dev = tensorf.aabb.device
    c2w = torch.as_tensor(c2w, dtype=torch.float32).to(dev)
    if torch.is_tensor(focal) and focal.device != dev:
        focal = focal.to(dev)
    rays = camera_rays(c2w.reshape(1, 3, 4), focal, H, W, ndc=ray_type == "ndc", near=1.0)
    ts = torch.full((H * W,), float(t), device=dev)
    req = None
    if motion:
        own = c2w.reshape(3, 4)
        req = dict(H=H, W=W, focal=focal, c2w_f=own if c2w_f is None else c2w_f, c2w_b=own if c2w_b is None else c2w_b,
                   maps=motion)
    return _render_image(tensorf_static, tensorf, rays, ts, H, W, N_samples, ray_type, chunk, maps, req, alpha_masks)


def _track_points_raw(tensorf, pts, ts, n_fwd, n_bwd, dt, cameras, focal, H, W, ray_type, want, bufs=None, ws=None):
    """rdrf_track_points_fwd on checked arguments.  want: subset of L.TRACK_OUTPUTS; bufs / ws: caller-owned output
    buffers by name and workspace (the tests poison them), else allocated here.  Returns the buffers by name."""
    L.require_device(pts, ts, cameras)
    pts, ts = L.f32c(pts.detach()), L.f32c(ts.detach())
    M, K, dev = pts.shape[0], n_bwd + 1 + n_fwd, pts.device
    shapes = {"pts": (M, K, 3), "pix": (M, K, 2), "disp": (M, K)}
    if bufs is None:
        bufs = {n: torch.empty(shapes[n], device=dev) for n in want}
    keep = None
    cams = None
    if cameras is not None:
        cameras = L.f32c(cameras.detach())
        f = _focal_tensor(focal.detach().to(dev) if torch.is_tensor(focal) else focal, dev).contiguous()
        cams = L.TrackCamsC(int(H), int(W), int(cameras.shape[0]), f.data_ptr(), cameras.data_ptr())
        keep = (cameras, f)
    out = L.TracksC(*[bufs[n].data_ptr() if n in want else None for n in L.TRACK_OUTPUTS])
    P, cfg = field_structs(tensorf, tensorf._param_list(), ray_type)
    if ws is None:
        ws = L.workspace(dev, L.lib.rdrf_track_ws_bytes(M, K))
    L.check(L.lib.rdrf_track_points_fwd(C.byref(P), C.byref(cfg), L.ptr(pts), L.ptr(ts), M, int(n_fwd), int(n_bwd), dt,
                                        None if cams is None else C.byref(cams), C.byref(out), L.ptr(ws), ws.numel(),
                                        L.stream_of(pts)), "rdrf_track_points_fwd")
    del keep
    return bufs


def _track_args(pts, ts, n_fwd, n_bwd, T, cameras, focal, H, W, ray_type):
    """argument checks of track_points (before any device work); returns (n_fwd, n_bwd, dt)"""
    if ray_type not in L.RAY_TYPES:
        raise NotImplementedError("track_points: ray_type must be 'ndc' or 'contract' (the reference projects no other, "
                                  "renderer.py:1335-1351)")
    n_fwd, n_bwd = int(n_fwd), int(n_bwd)
    if n_fwd < 0 or n_bwd < 0:
        raise ValueError(f"track_points: n_fwd and n_bwd are step counts >= 0, got {n_fwd}, {n_bwd}")
    if pts.dim() != 2 or pts.shape[1] != 3 or ts.shape != pts.shape[:1]:
        raise ValueError("track_points: pts [M,3] un-normalised field coordinates, ts [M] times in [-1,1]")
    if int(T) < 2 and (n_fwd or n_bwd):
        raise ValueError("track_points: a video of T < 2 frames has no time step")
    if cameras is not None:
        K = n_bwd + 1 + n_fwd
        if cameras.dim() != 3 or tuple(cameras.shape[1:]) != (3, 4) or cameras.shape[0] != K:
            raise ValueError(f"track_points: cameras must be [K,3,4] with K = n_bwd + 1 + n_fwd = {K}, got {tuple(cameras.shape)}")
        if focal is None or H is None or W is None or int(H) <= 0 or int(W) <= 0:
            raise ValueError("track_points: cameras need focal, H and W")
    return n_fwd, n_bwd, (2.0 / (int(T) - 1) if int(T) >= 2 else 0.0)


@torch.no_grad()
def track_points(tensorf, pts, ts, n_fwd, n_bwd, T, cameras=None, focal=None, H=None, W=None, ray_type="ndc"):
    """Follow M points through the video by chaining the scene-flow field natively (rdrf_track_points_fwd, ONE launch):
    pts [M,3] un-normalised field coordinates (as get_forward_backward_scene_flow takes them) at times ts [M] in [-1,1],
    n_fwd steps p + scene_flow_f forward and n_bwd steps p + scene_flow_b backward, the time moving by 2 / (T - 1) per
    step; contract scenes clamp every step to [-2 + 1e-6, 2 - 1e-6] (train.py:1377-1378).  Bit for bit the chain of
    get_forward_backward_scene_flow_point_single calls.  cameras [K,3,4] (K = n_bwd + 1 + n_fwd, camera k of slot k) with
    focal, H, W: each point is projected into its slot's camera as render_single_3d_point does (contract:
    render_3d_point's contract2world leg).  Returns Tracks(points [M,K,3], pixels [M,K,2] | None, disp [M,K] | None,
    frames_offset [K]); slot n_bwd is the seed.  No gradients.  Whether slot k's camera sees the point: track_visibility."""
    n_fwd, n_bwd, dt = _track_args(pts, ts, n_fwd, n_bwd, T, cameras, focal, H, W, ray_type)
    want = L.TRACK_OUTPUTS if cameras is not None else ("pts",)
    b = _track_points_raw(tensorf, pts, ts, n_fwd, n_bwd, dt, cameras, focal, H, W, ray_type, want)
    return Tracks(b["pts"], b.get("pix"), b.get("disp"), torch.arange(-n_bwd, n_fwd + 1, device=pts.device))


def _track_vis_args(points, ts, n_fwd, n_bwd, T, cameras, focal, H, W, ray_type, margin):
    """argument checks of track_visibility (before any device work); returns (n_fwd, n_bwd, dt)"""
    if ray_type not in L.RAY_TYPES:
        raise NotImplementedError("track_visibility: ray_type must be 'ndc' or 'contract' (the reference projects no other, "
                                  "renderer.py:1335-1351)")
    n_fwd, n_bwd = int(n_fwd), int(n_bwd)
    if n_fwd < 0 or n_bwd < 0:
        raise ValueError(f"track_visibility: n_fwd and n_bwd are step counts >= 0, got {n_fwd}, {n_bwd}")
    K = n_bwd + 1 + n_fwd
    if not torch.is_tensor(points) or points.dim() != 3 or tuple(points.shape[1:]) != (K, 3):
        raise ValueError(f"track_visibility: points must be [M,K,3] with K = n_bwd + 1 + n_fwd = {K} (Tracks.points), got "
                         f"{tuple(points.shape) if torch.is_tensor(points) else type(points).__name__}")
    if not torch.is_tensor(ts) or ts.shape != points.shape[:1]:
        raise ValueError("track_visibility: ts [M] times of the seeds in [-1,1]")
    if int(T) < 2 and (n_fwd or n_bwd):
        raise ValueError("track_visibility: a video of T < 2 frames has no time step")
    if cameras is None or not torch.is_tensor(cameras) or cameras.dim() != 3 or tuple(cameras.shape) != (K, 3, 4):
        raise ValueError(f"track_visibility: cameras must be [K,3,4] with K = n_bwd + 1 + n_fwd = {K}, got "
                         f"{tuple(cameras.shape) if torch.is_tensor(cameras) else cameras!r}")
    if focal is None or H is None or W is None or int(H) <= 0 or int(W) <= 0:
        raise ValueError("track_visibility: cameras need focal, H and W")
    if not float(margin) == float(margin):
        raise ValueError("track_visibility: margin is a depth in z_vals units, got NaN")
    return n_fwd, n_bwd, (2.0 / (int(T) - 1) if int(T) >= 2 else 0.0)


def _track_vis_chunk(M, K, S, H, W):
    """points per rdrf_track_visibility_fwd call: as many as keep the workspace within what render_rays takes for one H x W
    frame of S samples (one point at least), and the 32-bit sample indices in range"""
    budget = int(L.lib.rdrf_render_workspace_bytes(int(H) * int(W), S))
    fixed = int(L.lib.rdrf_track_visibility_ws_bytes(0, K, S))
    per = max(int(L.lib.rdrf_track_visibility_ws_bytes(1024, K, S)) - fixed, 1) / 1024.0   # bytes per point (256-byte rounding aside)
    m = int(max(budget - fixed, 0) / per)
    m = min(m, (2 ** 31 - 1) // (3 * S * K) - 1)
    while m > 1 and int(L.lib.rdrf_track_visibility_ws_bytes(m, K, S)) > budget:
        m -= max(m // 64, 1)
    return max(1, min(m, max(M, 1)))


def _track_visibility_raw(tensorf_static, tensorf, points, ts, n_fwd, n_bwd, dt, cameras, focal, H, W, S, ray_type, margin,
                          vis=None, ws=None):
    """rdrf_track_visibility_fwd on checked arguments, ONE call for all M points.  vis / ws: caller-owned output buffer
    [M,K] and workspace (the tests poison them), else allocated here.  Returns vis."""
    L.require_device(points, ts, cameras)
    points, ts = L.f32c(points.detach()), L.f32c(ts.detach())
    M, K, dev = points.shape[0], n_bwd + 1 + n_fwd, points.device
    if vis is None:
        vis = torch.empty(M, K, device=dev)
    if M == 0:
        return vis
    cameras = L.f32c(cameras.detach().to(dev))
    f = _focal_tensor(focal.detach().to(dev) if torch.is_tensor(focal) else focal, dev).contiguous()
    cams = L.TrackCamsC(int(H), int(W), K, f.data_ptr(), cameras.data_ptr())
    PS, cs, PD, cd = render_structs(tensorf_static, tensorf, ray_type)
    if ws is None:
        ws = L.workspace(dev, L.lib.rdrf_track_visibility_ws_bytes(M, K, S))
    near, far = tensorf.near_far
    L.check(L.lib.rdrf_track_visibility_fwd(C.byref(PS), C.byref(cs), C.byref(PD), C.byref(cd), L.ptr(points), L.ptr(ts), M,
                                            int(n_fwd), int(n_bwd), dt, C.byref(cams), S, near, far, float(margin), L.ptr(vis),
                                            L.ptr(ws), ws.numel(), L.stream_of(points)), "rdrf_track_visibility_fwd")
    del cameras, f
    return vis


@torch.no_grad()
def track_visibility(tensorf_static, tensorf, tracks_or_points, ts, n_fwd, n_bwd, T, cameras, focal, H, W, N_samples=-1,
                     ray_type="ndc", margin=0.0):
    """Per-slot visibility of point tracks, natively (rdrf_track_visibility_fwd): vis [M,K], the transmittance T_full of
    raw2outputs (renderer.py:236-245) from camera k to the point of slot k.  tracks_or_points: a Tracks, or its points [M,K,3]
    (field coordinates); ts [M] the seeds' times, n_fwd, n_bwd, T as track_points takes them (slot k's time is the chain's);
    cameras [K,3,4] with focal, H, W: camera k of slot k.
    The slot's ray is camera k's ray through the slot's own fractional pixel (Tracks.pixels[i,k]), sampled by the field's
    no-jitter sampler with N_samples (default: the dynamic field's nSamples); sigma of both fields and the blending are
    forward()'s for that ray and time; vis is the compositor's product of (1 - alpha_d b)(1 - alpha_s (1 - b)) + 1e-10 over
    the samples in front of the query depth zq = z* - margin, the interval that holds zq counted for the part in front of it
    (at a sample position: T_full[j] of raw2outputs exactly; continuous in between).  z* is the point's depth on the ray in
    z_vals units: (clamp(p_z, -1, 1 - 1e-6) + 1) / 2 for ndc, -cam_z for contract.
    margin (z_vals units, default 0): a seed made by render_tracks sits inside the density that defines it, so at margin 0
    its value is well below 1; to ask "is the surface seen from camera k" pass a margin of a few sample steps (ndc: a step
    is (far - near) / (N_samples - 1)).
    zq in front of the first sample gives exactly 1, a point behind its camera exactly 0.  Pixels outside the frame are
    computed like any other: clip with Tracks.pixels.  Only the samples in front of the points reach a density kernel and no
    colour is computed.  A slot's bits do not depend on M or on the other slots; large M is processed in chunks of points
    whose workspace stays within render_rays' for one H x W frame.  No gradients."""
    points = tracks_or_points.points if isinstance(tracks_or_points, Tracks) else tracks_or_points
    n_fwd, n_bwd, dt = _track_vis_args(points, ts, n_fwd, n_bwd, T, cameras, focal, H, W, ray_type, margin)
    S = _n_samples(tensorf, N_samples)
    M, K = points.shape[0], n_bwd + 1 + n_fwd
    L.require_device(points, ts, cameras)
    vis = torch.empty(M, K, device=points.device)
    if M == 0:
        return vis
    chunk = _track_vis_chunk(M, K, S, H, W)
    for m0 in range(0, M, chunk):
        _track_visibility_raw(tensorf_static, tensorf, points[m0:m0 + chunk], ts[m0:m0 + chunk], n_fwd, n_bwd, dt, cameras,
                              focal, H, W, S, ray_type, margin, vis=vis[m0:m0 + chunk])
    return vis


def _hit_taus(tau, who):
    """the opacity levels of a hits call (checked before any device work) -> (list of floats, whether `tau` was a scalar)"""
    scalar = not isinstance(tau, (list, tuple)) and not (hasattr(tau, "__len__") and getattr(tau, "ndim", 1) > 0)
    taus = [float(tau)] if scalar else [float(t) for t in tau]
    if not 1 <= len(taus) <= L.HITS_MAX_TAU:
        raise ValueError(f"{who}: 1 to {L.HITS_MAX_TAU} opacity levels per call, got {len(taus)}")
    if any(not 0.0 < t < 1.0 for t in taus):
        raise ValueError(f"{who}: every tau must lie in (0, 1), got {taus}")
    if any(b <= a for a, b in zip(taus, taus[1:])):
        raise ValueError(f"{who}: the levels must ascend strictly, got {taus}")
    return taus, scalar


def _hits_chunk(N, S):
    """rays per rdrf_render_hits_fwd call: as many as keep the 32-bit sample indices in range (N S 3 < 2^31)"""
    return max(1, min(max(int(N), 1), (2 ** 31 - 1) // (3 * int(S)) - 1))


def _hits_struct(bufs):
    return L.HitsC(*[bufs[n].data_ptr() if n in bufs else None for n in L.HIT_OUTPUTS])


def _alloc_hits(n_tau, N, dev, want=L.HIT_OUTPUTS):
    shapes = {"z": (n_tau, N), "hit": (n_tau, N), "xyz": (n_tau, N, 3), "owner": (n_tau, N)}
    return {n: torch.empty(shapes[n], device=dev, dtype=torch.uint8 if n == "hit" else torch.float32) for n in want}


def _render_hits_raw(tensorf_static, tensorf, rays, ts, taus, S, ray_type, map_names, bufs=None, mbufs=None, ws=None):
    """rdrf_render_hits_fwd on checked arguments, ONE call for all N rays.  map_names: the RenderMaps fields to write (empty:
    the density-only path).  bufs / mbufs / ws: caller-owned hit buffers [n_tau,N..] and map buffers by name and workspace
    (the tests poison them), else allocated here.  Returns (bufs, mbufs)."""
    L.require_device(rays, ts)
    rays, ts = L.f32c(rays), L.f32c(ts)
    N, dev = rays.shape[0], rays.device
    if bufs is None:
        bufs = _alloc_hits(len(taus), N, dev)
    if mbufs is None:
        mbufs = _alloc_maps(map_names, N, dev)
    if N == 0:
        return bufs, mbufs
    PS, cs, PD, cd = render_structs(tensorf_static, tensorf, ray_type)
    if ws is None:
        ws = L.workspace(dev, L.lib.rdrf_render_hits_ws_bytes(N, S))
    near, far = tensorf.near_far
    arr = (C.c_float * len(taus))(*taus)
    Mp = _maps_struct(mbufs) if map_names else None
    out = _hits_struct(bufs)
    L.check(L.lib.rdrf_render_hits_fwd(C.byref(PS), C.byref(cs), C.byref(PD), C.byref(cd), L.ptr(rays), L.ptr(ts), N, S, near, far,
                                       arr, len(taus), None if Mp is None else C.byref(Mp), C.byref(out), L.ptr(ws), ws.numel(),
                                       L.stream_of(rays)), "rdrf_render_hits_fwd")
    return bufs, mbufs


def hits_from_planes(rays, z, sigma_s, sigma_d, blending, tau=0.5, ray_type="ndc", distance_scale=1.0):
    """rdrf_hits_from_planes: the hits kernel alone on the caller's device planes z, sigma_s, sigma_d, blending [N,S] of the
    rays [N,6] (dists are formed from z and the ray norm as the fields form them).  Returns the dict of render_hits without
    maps."""
    taus, scalar = _hit_taus(tau, "hits_from_planes")
    if ray_type not in L.RAY_TYPES:
        raise NotImplementedError("hits_from_planes: ray_type must be 'ndc' or 'contract'")
    L.require_device(rays, z, sigma_s, sigma_d, blending)
    rays, z, sigma_s, sigma_d, blending = (L.f32c(t) for t in (rays, z, sigma_s, sigma_d, blending))
    N, S = z.shape
    if rays.shape != (N, 6) or any(t.shape != (N, S) for t in (sigma_s, sigma_d, blending)):
        raise ValueError("hits_from_planes: rays [N,6]; z, sigma_s, sigma_d, blending [N,S]")
    bufs = _alloc_hits(len(taus), N, z.device)
    out = _hits_struct(bufs)
    arr = (C.c_float * len(taus))(*taus)
    L.check(L.lib.rdrf_hits_from_planes(L.ptr(rays), L.ptr(z), L.ptr(sigma_s), L.ptr(sigma_d), L.ptr(blending), N, S,
                                        L.RAY_TYPES[ray_type], float(distance_scale), arr, len(taus), C.byref(out),
                                        L.stream_of(z)), "rdrf_hits_from_planes")
    return _hits_result(bufs, {}, scalar)


def _hits_result(bufs, mbufs, scalar):
    out = {n: (bufs[n][0] if scalar else bufs[n]) for n in L.HIT_OUTPUTS}
    out["hit"] = out["hit"].bool()
    out.update(mbufs)
    return out


@torch.no_grad()
def render_hits(tensorf_static, tensorf, rays, ts, tau=0.5, N_samples=-1, ray_type="ndc", maps=False):
    """Surface hits of a ray batch, natively (rdrf_render_hits_fwd): per ray the depth at which the opacity 1 - T_full of
    raw2outputs (renderer.py:236-245) reaches `tau` -- tau = 0.5 is the median depth -- where the depth maps of render_rays
    are expected depths, which lie between the surfaces at an occlusion edge and inside a floater.
    Returns a dict: z [N] the hit depth in z_vals units (between the two samples the crossing lies in, exact for the
    compositor's piecewise-constant density), hit [N] bool (False: the ray never gets that opaque; z is then the last
    sample's depth), xyz [N,3] the point at z in field coordinates (the sampler's arithmetic, as sampleXYZ's xyz), owner [N]
    the dynamic field's share of the hit sample (1: a moving surface, 0: the static scene).  `tau` may be a sequence of up
    to 8 strictly ascending levels in (0, 1): every output gains a leading axis, and all levels come from one scan.
    maps: False -- the density-only path, no colour is computed --, or True / a subset of the RenderMaps field names: the
    render runs as render_rays(maps=...) does and the dict also holds those maps by name, bit for bit.  Both paths give the
    same hits.  A ray's bits do not depend on the batch: large N is processed in chunks.  ndc or contract; no gradients."""
    taus, scalar = _hit_taus(tau, "render_hits")
    if ray_type not in L.RAY_TYPES:
        raise NotImplementedError("render_hits: ray_type must be 'ndc' or 'contract' (world-space rays are not built here)")
    names = _map_names(maps) if maps else ()
    L.require_device(rays, ts)
    N, dev = rays.shape[0], rays.device
    S = _n_samples(tensorf, N_samples)
    chunk = _hits_chunk(N, S)
    if chunk >= N:
        bufs, mbufs = _render_hits_raw(tensorf_static, tensorf, rays, ts, taus, S, ray_type, names)
        return _hits_result(bufs, mbufs, scalar)
    bufs, mbufs = _alloc_hits(len(taus), N, dev), _alloc_maps(names, N, dev)
    for c0 in range(0, N, chunk):
        b, m = _render_hits_raw(tensorf_static, tensorf, rays[c0:c0 + chunk], ts[c0:c0 + chunk], taus, S, ray_type, names)
        for n in bufs:
            bufs[n][:, c0:c0 + chunk] = b[n]
        for n in mbufs:
            mbufs[n][c0:c0 + chunk] = m[n]
    return _hits_result(bufs, mbufs, scalar)


@torch.no_grad()
def hit_view(tensorf_static, tensorf, c2w, focal, H, W, t, tau=0.5, N_samples=-1, ray_type="ndc", maps=False):
    """render_hits on the rays of one camera c2w [3,4] at time t in [-1,1] (camera_rays, as render_view): the same dict as
    images -- z, hit, owner [H,W], xyz [H,W,3] (a leading level axis for a sequence of taus), maps [H,W] / [H,W,3], raw."""
    taus, scalar = _hit_taus(tau, "hit_view")
    if ray_type not in L.RAY_TYPES:
        raise NotImplementedError("hit_view: ray_type must be 'ndc' or 'contract' (world-space rays are not built here)")
    dev = tensorf.aabb.device
    c2w = torch.as_tensor(c2w, dtype=torch.float32).to(dev)
    if torch.is_tensor(focal) and focal.device != dev:
        focal = focal.to(dev)
    rays = camera_rays(c2w.reshape(1, 3, 4), focal, H, W, ndc=ray_type == "ndc", near=1.0)
    ts = torch.full((H * W,), float(t), device=dev)
    out = render_hits(tensorf_static, tensorf, rays, ts, taus[0] if scalar else taus, N_samples, ray_type, maps)

    def image(n, v):
        k = 1 if n in L.HIT_OUTPUTS and not scalar else 0   # the level axis stays in front
        return v.view(*v.shape[:k], H, W, *v.shape[k + 1:])

    return {n: image(n, v) for n, v in out.items()}


@torch.no_grad()
def render_tracks(tensorf_static, tensorf, poses9, focal, frame, pixels, H, W, span=None, N_samples=-1, ray_type="ndc"):
    """Tracks of M query pixels of `frame`: pixels [M,2] integer (column, row).  Their rays are rendered by the no-grad
    launch sequence (rdrf_render_track_seeds_fwd), the seed of a pixel is render_3d_point's point
    sum_s weights_d xyz + (1 - acc_d) far of its ray, and track_points follows it through the frames
    frame - span .. frame + span clipped to [0, T - 1] (span None: the whole video; a pair: (backward, forward)), projected
    into those frames' cameras.  Returns (Tracks, acc_d [M]): a seed with a small acc_d sits in static or empty space.
    Their visibility: track_visibility(tensorf_static, tensorf, tracks, ts, n_fwd, n_bwd, T, cameras, ...) with ts = the
    frame's time 2 frame / (T - 1) - 1 for every pixel, n_bwd = -frames_offset[0], n_fwd = frames_offset[-1] and
    cameras = pose_to_mtx(poses9)[frame - n_bwd: frame + n_fwd + 1] (see there: a seed sits inside its own density, so pass a
    margin of a few sample steps).  Seeds ON the surface: render_hit_tracks."""
    return _render_tracks(tensorf_static, tensorf, poses9, focal, frame, pixels, H, W, span, N_samples, ray_type, None)


@torch.no_grad()
def render_hit_tracks(tensorf_static, tensorf, poses9, focal, frame, pixels, H, W, span=None, N_samples=-1, ray_type="ndc",
                      tau=0.5):
    """render_tracks with the seeds on the surface: the seed of a pixel is the surface hit of its ray at the opacity level
    `tau` (render_hits' xyz: where the ray's opacity reaches tau, not a blend of depths inside the density), and a ray that
    misses keeps render_tracks' expected-depth seed.  Same arguments and returns otherwise: (Tracks, acc_d [M])."""
    taus, scalar = _hit_taus(tau, "render_hit_tracks")
    if not scalar:
        raise ValueError("render_hit_tracks: one opacity level seeds the tracks")
    return _render_tracks(tensorf_static, tensorf, poses9, focal, frame, pixels, H, W, span, N_samples, ray_type, taus[0])


def _render_tracks(tensorf_static, tensorf, poses9, focal, frame, pixels, H, W, span, N_samples, ray_type, tau):
    """render_tracks (tau None) / render_hit_tracks (the seeds' opacity level)"""
    from .ray_utils import generate_rays, pose_to_mtx
    if ray_type not in L.RAY_TYPES:
        raise NotImplementedError("render_tracks: ray_type must be 'ndc' or 'contract' (the reference projects no other, "
                                  "renderer.py:1335-1351)")
    T, frame = poses9.shape[0], int(frame)
    if not 0 <= frame < T:
        raise ValueError(f"render_tracks: frame {frame} of a {T}-frame video")
    sb, sf_ = (T, T) if span is None else ((int(span[0]), int(span[1])) if isinstance(span, (tuple, list)) else (int(span), int(span)))
    if sb < 0 or sf_ < 0:
        raise ValueError("render_tracks: span >= 0")
    n_bwd, n_fwd = min(sb, frame), min(sf_, T - 1 - frame)
    L.require_device(poses9, pixels)
    dev = poses9.device
    pixels = pixels.to(dev).long()
    if pixels.dim() != 2 or pixels.shape[1] != 2:
        raise ValueError("render_tracks: pixels [M,2] integer (column, row)")
    M = pixels.shape[0]
    ids = pixels[:, 1] * W + pixels[:, 0] + frame * H * W
    rays = L.f32c(generate_rays(ids, poses9, focal, H, W, ndc=ray_type == "ndc", near=1.0))
    ts = torch.full((M,), 2.0 * frame / max(T - 1, 1) - 1.0, device=dev)
    S = _n_samples(tensorf, N_samples)
    seeds = torch.empty(M, 3, device=dev)
    bufs = _alloc_maps(("acc_d",), M, dev)
    if M:
        ws = L.workspace(dev, L.lib.rdrf_render_motion_workspace_bytes(M, S))
        PS, cs, PD, cd = render_structs(tensorf_static, tensorf, ray_type)
        near, far = tensorf.near_far
        Mp = _maps_struct(bufs)
        L.check(L.lib.rdrf_render_track_seeds_fwd(C.byref(PS), C.byref(cs), C.byref(PD), C.byref(cd), L.ptr(rays), L.ptr(ts), M, S,
                                                  near, far, C.byref(Mp), L.ptr(seeds), L.ptr(ws), ws.numel(),
                                                  L.stream_of(rays)), "rdrf_render_track_seeds_fwd")
        if tau is not None:
            h = render_hits(tensorf_static, tensorf, rays, ts, tau, S, ray_type)
            seeds = torch.where(h["hit"][:, None], h["xyz"], seeds)
    cams =pose_to_mtx(poses9.detach().float())[frame - n_bwd: frame + n_fwd + 1]
    tracks = track_points(tensorf, seeds, ts, n_fwd, n_bwd, T, cameras=cams, focal=focal, H=H, W=W, ray_type=ray_type)
    return tracks, bufs["acc_d"]


def flow_to_image(flow):
    """flow_viz.flow_to_image with its defaults (flow_viz.py:107-136) on the device (rdrf_flow_to_image): flow [H,W,2] ->
    uint8 [H,W,3] RGB of the Middlebury colour wheel, in numpy's precision sequence.  The input is not modified."""
    L.require_device(flow)
    if flow.dim() != 3 or flow.shape[2] != 2:
        raise L.RdrfError(f"flow_to_image: flow must be [H,W,2], got {tuple(flow.shape)}")
    flow = L.f32c(flow.detach())
    H, W, _ = flow.shape
    rgb = torch.empty(H, W, 3, dtype=torch.uint8, device=flow.device)
    if H * W == 0:
        return rgb
    ws = L.workspace(flow.device, int(L.lib.rdrf_flow_to_image_workspace_bytes(H, W)))
    L.check(L.lib.rdrf_flow_to_image(L.ptr(flow), H, W, L.ptr(rgb), L.ptr(ws), ws.numel(), L.stream_of(flow)),
            "rdrf_flow_to_image")
    return rgb


def delta_xyz_image(delta_xyz):
    """renderer.py:611-613: the warp-displacement map as a picture, (d / max|d| + 1) / 2"""
    return (delta_xyz / torch.max(torch.abs(delta_xyz)) + 1.0) / 2.0


def path_time(change_time, idx, n):
    """evaluation_path's time of view idx of n (renderer.py:1034-1043): "change" walks the path's own time axis,
    round(idx / (n - 1) * (n - 1)) / (n - 1) * 2 - 1 (a one-view path: -1, the first time instance); a number is
    that time for every view."""
    if isinstance(change_time, str):
        if change_time != "change":
            raise ValueError(f"change_time: 'change' or a time in [-1, 1], got {change_time!r}")
        return round(idx / (n - 1) * (n - 1)) / (n - 1) * 2.0 - 1.0 if n > 1 else -1.0
    return float(change_time)


def render_path(tensorf_static, tensorf, c2ws, focal, H, W, change_time="change", N_samples=-1, ray_type="ndc",
                maps=True, chunk=None, alpha_masks=None):
    """renderer.py:970-1263 `evaluation_path`: yields render_view(c2ws[idx], focal[idx] or focal, path_time(...)) per
    view, in order.  c2ws [n,3,4] (a tensor, an array or a list of [3,4]); focal a scalar or one per view (render_focal);
    change_time "change" or a fixed time (path_time).  The image / video writing is the caller's.  `alpha_masks`: as
    render_rays."""
    n = len(c2ws)
    per_view = (torch.is_tensor(focal) and focal.numel() > 1) or (not torch.is_tensor(focal) and hasattr(focal, "__len__"))
    if per_view and len(focal) != n:
        raise ValueError(f"render_path: {len(focal)} focal values for {n} views")
    for idx in range(n):
        yield render_view(tensorf_static, tensorf, c2ws[idx], focal[idx] if per_view else focal, H, W,
                          path_time(change_time, idx, n), N_samples, ray_type, maps, chunk, alpha_masks=alpha_masks)


def psnr(img, ref):
    """-10 log10(mse) on the device (renderer.py:905-906 computes it per image on the host)."""
    return -10.0 * torch.log10(((img - ref) ** 2).mean())


def ssim(img, ref, max_val=1.0, return_map=False):
    """utils.py:98-151 rgb_ssim with its defaults (11-tap Gaussian, sigma 1.5, k1 0.01, k2 0.03) on the device
    (rdrf_ssim; the reference runs scipy on the host per image): img, ref [H,W,C] device tensors, H, W >= 11.  Moments,
    map and mean in fp64 (the products of the pixels included).  Returns the mean as a 0-d fp64 tensor, or with
    `return_map` the map [H-10,W-10,C] (fp32), as rgb_ssim does."""
    L.require_device(img, ref)
    if img.dim() != 3 or img.shape != ref.shape:
        raise L.RdrfError(f"ssim: img and ref must be [H,W,C] of one shape, got {tuple(img.shape)} and {tuple(ref.shape)}")
    H, W, Cc = img.shape
    if H < 11 or W < 11 or Cc < 1:
        raise L.RdrfError(f"ssim: the images ({H} x {W}) must be at least 11 x 11 (valid 11-tap filter)")
    img, ref = L.f32c(img), L.f32c(ref)
    dev = img.device
    mean = torch.empty((), dtype=torch.float64, device=dev)
    smap = torch.empty(H - 10, W - 10, Cc, device=dev) if return_map else None
    ws = L.workspace(dev, int(L.lib.rdrf_ssim_workspace_bytes(H, W, Cc)))
    L.check(L.lib.rdrf_ssim(L.ptr(img), L.ptr(ref), H, W, Cc, float(max_val), L.ptr(mean), L.ptr(smap), L.ptr(ws), ws.numel(),
                            L.stream_of(img)), "rdrf_ssim")
    return smap if return_map else mean


# --------------------------------------------------------------------------------------------
# induced optical flow / disparity (renderer.py:1266-1392) -- SURVEY.md 8f rank 1
# --------------------------------------------------------------------------------------------
def _focal_tensor(focal, dev):
    if torch.is_tensor(focal):
        L.require_device(focal)
        return focal.reshape(1).float()
    return torch.full((1,), float(focal), device=dev)


class _InduceFlowFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, H, W, focal, c2w, weights, pts, pts_2d, rays, ray_type):
        ctx.set_materialize_grads(False)
        L.require_device(c2w, weights, pts, pts_2d, rays)
        c2w, weights, pts, pts_2d, rays = (L.f32c(t) for t in (c2w, weights, pts, pts_2d, rays))
        focal = L.f32c(focal)
        N, S = weights.shape
        if c2w.shape != (N, 3, 4) or pts.shape != (N, S, 3) or rays.shape != (N, 6) or pts_2d.shape != (N, 2):
            raise L.RdrfError("induce_flow: expected pose [N,3,4], weights [N,S], pts [N,S,3], pts_2d [N,2], "
                              "rays [N,6]")
        if ray_type not in ("ndc", "contract"):
            raise L.RdrfError("induce_flow: ray_type must be 'ndc' or 'contract' (renderer.py:1343-1361)")
        flow = torch.empty(N, 2, device=weights.device)
        disp = torch.empty(N, 1, device=weights.device)
        L.check(L.lib.rdrf_induce_flow_fwd(int(H), int(W), L.ptr(focal), L.ptr(c2w), L.ptr(weights),
                                           L.ptr(pts), L.ptr(pts_2d), L.ptr(rays), N, S,
                                           L.RAY_TYPES[ray_type], L.ptr(flow), L.ptr(disp),
                                           L.stream_of(weights)), "rdrf_induce_flow_fwd")
        ctx.hw, ctx.ray_type = (int(H), int(W)), ray_type
        ctx.save_for_backward(focal, c2w, weights, pts, rays)
        return flow, disp

    @staticmethod
    def backward(ctx, g_flow, g_disp):
        focal, c2w, weights, pts, rays = ctx.saved_tensors
        N, S = weights.shape
        need = ctx.needs_input_grad     # H, W, focal, c2w, weights, pts, pts_2d, rays, ray_type
        g_focal, g_c2w, g_w, g_pts, g_rays = L.zeros_like_many([focal, c2w, weights, pts, rays],
                                                               [need[2], need[3], need[4], need[5], need[7]])
        g_flow = None if g_flow is None else L.f32c(g_flow)
        g_disp = None if g_disp is None else L.f32c(g_disp)
        L.check(L.lib.rdrf_induce_flow_bwd(ctx.hw[0], ctx.hw[1], L.ptr(focal), L.ptr(c2w), L.ptr(weights),
                                           L.ptr(pts), L.ptr(rays), N, S, L.RAY_TYPES[ctx.ray_type],
                                           L.ptr(g_flow), L.ptr(g_disp), L.ptr(g_w), L.ptr(g_pts),
                                           L.ptr(g_rays), L.ptr(g_c2w), L.ptr(g_focal),
                                           L.stream_of(weights)), "rdrf_induce_flow_bwd")
        g_p2d = None if (not need[6] or g_flow is None) else -g_flow
        return (None, None, g_focal, g_c2w, g_w, g_pts, g_p2d, g_rays, None)


def render_3d_point(H, W, f, c2w, weights, pts, rays, ray_type="ndc"):
    """renderer.py:1334-1378: weight-averaged 3-D point along each ray, projected into the camera
    c2w [N,3,4]; returns (pixel coordinates [N,2], NDC depth [N,1])."""
    dev = weights.device
    zero = torch.zeros(weights.shape[0], 2, device=dev)
    flow, disp = _InduceFlowFn.apply(H, W, _focal_tensor(f, dev), c2w, weights, pts, zero, rays, ray_type)
    return flow, disp


def induce_flow(H, W, focal, pose_neighbor, weights, pts_3d_neighbor, pts_2d, rays, ray_type="ndc"):
    """renderer.py:1381-1392: (induced_flow [N,2], induced_disp [N,1])."""
    return _InduceFlowFn.apply(H, W, _focal_tensor(focal, weights.device), pose_neighbor, weights,
                               pts_3d_neighbor, pts_2d, rays, ray_type)


def render_single_3d_point(H, W, f, c2w, pt_NDC):
    """renderer.py:1301-1331: the S = 1, weight 1 case; disparity is returned as (z_ndc + 1) / 2."""
    N = pt_NDC.shape[0]
    dev = pt_NDC.device
    one = torch.ones(N, 1, device=dev)
    plane, d = _InduceFlowFn.apply(H, W, _focal_tensor(f, dev), c2w, one, pt_NDC.reshape(N, 1, 3),
                                   torch.zeros(N, 2, device=dev), torch.zeros(N, 6, device=dev), "ndc")
    return plane, (d + 1.0) / 2.0


def induce_flow_single(H, W, focal, pose_neighbor, pts_3d_neighbor, pts_2d):
    """renderer.py:1381-1386 (induce_flow_single)."""
    return render_single_3d_point(H, W, focal, pose_neighbor, pts_3d_neighbor)[0] - pts_2d


# --------------------------------------------------------------------------------------------
# distortion loss (train.py:19-23 imports it from torch_efficient_distloss)
# --------------------------------------------------------------------------------------------
class _DistLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, w, m, interval):
        L.require_device(w, m)
        w, m = L.f32c(w), L.f32c(m)
        N, S = w.shape
        ipt = None
        if torch.is_tensor(interval):
            if interval.numel() == 1:
                interval = float(interval)
            else:
                L.require_device(interval)
                ipt, interval = L.f32c(interval).reshape(N, S), 0.0
        loss_ray = torch.empty(N, device=w.device)
        L.check(L.lib.rdrf_distloss_fwd(L.ptr(w), L.ptr(m), float(interval), L.ptr(ipt), N, S,
                                        L.ptr(loss_ray), L.stream_of(w)), "rdrf_distloss_fwd")
        ctx.interval, ctx.ipt = float(interval), ipt
        ctx.save_for_backward(w, m)
        return loss_ray

    @staticmethod
    def backward(ctx, g_ray):
        w, m = ctx.saved_tensors
        N, S = w.shape
        g_w = torch.zeros_like(w)
        L.check(L.lib.rdrf_distloss_bwd(L.ptr(w), L.ptr(m), ctx.interval, L.ptr(ctx.ipt), N, S,
                                        L.ptr(L.f32c(g_ray)), L.ptr(g_w), L.stream_of(w)), "rdrf_distloss_bwd")
        return g_w, None, None


def distloss_rays(w, m, interval):
    """the per-ray values of eff_distloss [N] (their mean is the loss): lets the trainer fold the mean and the loss
    weight into its fused loss reduction instead of three scalar launches per call"""
    return _DistLossFn.apply(w, m, interval)


def eff_distloss(w, m, interval):
    """torch_efficient_distloss.eff_distloss: w, m [N,S] (m ascending along a ray), interval a scalar
    or [N,S]; mean over rays of  sum_ij w_i w_j |m_i - m_j| + (1/3) sum_i interval w_i^2."""
    return _DistLossFn.apply(w, m, interval).sum() / w.shape[0]


def flatten_eff_distloss(w, m, interval, ray_id, n_rays=None):
    """torch_efficient_distloss.flatten_eff_distloss as the reference calls it (train.py:1299-1312):
    flattened [N*S] points with ray_id = tile(arange(N), S).  Only that regular layout is built;
    `n_rays` (= ray_id.max() + 1) may be passed to avoid the device->host read."""
    if n_rays is None:
        n_rays = int(ray_id.max().item()) + 1
        S = w.numel() // n_rays
        if w.numel() != n_rays * S or not bool((ray_id.reshape(n_rays, S)
                                                 == torch.arange(n_rays, device=ray_id.device)[:, None]).all()):
            raise NotImplementedError("flatten_eff_distloss: only ray_id = tile(arange(N), S) is built")
    S = w.numel() // n_rays
    if torch.is_tensor(interval) and interval.numel() > 1:
        interval = interval.reshape(n_rays, S)
    return _DistLossFn.apply(w.reshape(n_rays, S), m.reshape(n_rays, S), interval).sum() / n_rays
