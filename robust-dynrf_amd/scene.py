"""A training set built from arrays, resident on the device, with the interface of step.SyntheticScene.

The reference keeps every per-pixel tensor of the video as a flat (T*H*W, ...) tensor and indexes each of them with the
iteration's ray indices (train.py:951-990, 1043-1060).  Scene keeps the same tables, smaller:

    colours     uint8 input stays uint8 (converted as float(x) / 255 when a batch is cut), float32 stays float32
    masks       foreground, forward-flow and backward-flow masks as bits 0, 1, 2 of ONE byte per pixel
    nothing     for pixel centre, integer pixel, frame index and time: they are arithmetic on the index

and cuts a batch with one launch (rdrf_gather_batch) that writes every tensor of make_batch's dict.  The values are
bit-identical to gathers from float32 tables built on the host the way SyntheticScene builds its own (a uint8 colour x
is x / 255 in true fp32 division, view * (2 / (T - 1)) - 1 with the factor rounded to fp32 first).

The sampler has the semantics of the reference's SimpleSampler (train.py:81-93; two independent instances,
:1011-1012): every epoch is a fresh permutation of the pixels, cut into total // bs batches, the tail dropped.  It keeps
no cursor: batch(it, bs, which) is a pure function of (seed, which, it, bs), so a captured iteration, every data-parallel
rank and a resumed run draw the same indices.  File reading (images, RAFT flow, DPT disparity) is the caller's.
"""
import collections
import ctypes as C
import math

import numpy as np
import torch

from . import _lib as L
from .renderer import psnr, render_frame, render_view, ssim

FG_BIT, MASK_F_BIT, MASK_B_BIT = 1, 2, 4
# the fp32 outputs of one batch and their row widths: slices of one buffer (make_batch)
_BATCH_WIDTHS = (("rgb", 3), ("flow_f", 2), ("flow_b", 2), ("grid", 2), ("px", 2), ("disp", 1), ("fg", 1), ("mask_f", 1),
                 ("mask_b", 1), ("ts", 1), ("ts_rand", 1))


def _tensor(x, name):
    if x is None:
        raise ValueError(f"Scene: {name} is required")
    return torch.as_tensor(x)


def _mask_bits(m, name, shape):
    """[T,H,W] bool / integer (non-zero = set) / float (>= 0.5 = set) -> flat bool"""
    m = torch.as_tensor(m)
    if m.dim() == 4 and m.shape[-1] == 1:
        m = m[..., 0]
    if tuple(m.shape) != shape:
        raise ValueError(f"Scene: {name} must be [T,H,W] = {list(shape)}, got {list(m.shape)}")
    if m.dtype == torch.bool:
        return m.reshape(-1)
    return (m >= 0.5).reshape(-1) if m.is_floating_point() else (m != 0).reshape(-1)


def pack_poses(c2w):
    """camera-to-world matrices [T,3,4] -> the nine-number rows of the trainer's pose table: columns 0, 1 and 3 of
    every matrix (train.py:964-968; ray_utils.pose_to_mtx rebuilds column 2 as the cross product)"""
    c2w = torch.as_tensor(c2w, dtype=torch.float32)
    if c2w.dim() != 3 or tuple(c2w.shape[1:]) != (3, 4):
        raise ValueError(f"poses must be [T,3,4] camera-to-world matrices, got {list(c2w.shape)}")
    return torch.cat([c2w[:, :, 0], c2w[:, :, 1], c2w[:, :, 3]], -1)


class Scene:
    def __init__(self, rgb, flow_f, flow_b, flow_mask_f, flow_mask_b, disp=None, fg_mask=None, poses=None, focal=None,
                 heldout=None, device="cuda", seed=20211202):
        """rgb [T,H,W,3] uint8 or float32 in [0,1]; flow_f / flow_b [T,H,W,2] float32, pixels; flow_mask_f / flow_mask_b /
        fg_mask [T,H,W] bool, integer (non-zero = set) or float (>= 0.5 = set); disp [T,H,W] float32; poses [T,3,4]
        camera-to-world (None: the identity initialisation of train.py:970-971, for runs that optimise the poses); focal in
        pixels (None: the 30 degree half field of view the optimised one starts from, train.py:976-979); heldout: a list of
        (c2w [3,4], t in [-1,1], image [H,W,3]) for evaluate().  Arrays or tensors; everything is copied to `device`."""
        rgb = _tensor(rgb, "rgb")
        if rgb.dim() != 4 or rgb.shape[-1] != 3:
            raise ValueError(f"Scene: rgb must be [T,H,W,3], got {list(rgb.shape)}")
        if rgb.dtype not in (torch.uint8, torch.float32):
            raise ValueError(f"Scene: rgb must be uint8 or float32, got {rgb.dtype}")
        T, H, W = (int(v) for v in rgb.shape[:3])
        if T < 2:
            raise ValueError("Scene: at least two frames (the time axis is 2 / (T - 1) wide)")
        self.T, self.H, self.W = T, H, W
        self.total = T * H * W
        self.device = torch.device(device)
        self.seed = int(seed)
        dev = self.device
        flows = []
        for name, f in (("flow_f", flow_f), ("flow_b", flow_b)):
            f = _tensor(f, name)
            if tuple(f.shape) != (T, H, W, 2):
                raise ValueError(f"Scene: {name} must be [T,H,W,2] = {[T, H, W, 2]}, got {list(f.shape)}")
            flows.append(f.to(torch.float32).reshape(-1, 2).contiguous().to(dev))
        self.flow_f, self.flow_b = flows
        if flow_mask_f is None or flow_mask_b is None:
            raise ValueError("Scene: flow_mask_f and flow_mask_b are required")
        bits = _mask_bits(flow_mask_f, "flow_mask_f", (T, H, W)).to(torch.uint8) * MASK_F_BIT
        bits += _mask_bits(flow_mask_b, "flow_mask_b", (T, H, W)).to(torch.uint8) * MASK_B_BIT
        self.has_fg = fg_mask is not None
        if self.has_fg:
            bits += _mask_bits(fg_mask, "fg_mask", (T, H, W)).to(torch.uint8) * FG_BIT
        self.masks = bits.contiguous().to(dev)
        self.rgb = rgb.reshape(-1, 3).contiguous().to(dev)
        self.disp = None
        if disp is not None:
            disp = torch.as_tensor(disp)
            if tuple(disp.shape) != (T, H, W):
                raise ValueError(f"Scene: disp must be [T,H,W] = {[T, H, W]}, got {list(disp.shape)}")
            self.disp = disp.to(torch.float32).reshape(-1).contiguous().to(dev)
        self.has_poses = poses is not None
        if self.has_poses:
            p9 = pack_poses(poses)
            if p9.shape[0] != T:
                raise ValueError(f"Scene: {p9.shape[0]} poses for {T} frames")
        else:
            p9 = torch.zeros(T, 9)
            p9[:, 0] = 1.0
            p9[:, 4] = 1.0
        self.poses = p9.to(dev)
        focal = max(H, W) / 2.0 * math.sqrt(3.0) if focal is None else float(np.asarray(focal).reshape(-1)[0])
        self.focal = torch.tensor(focal, dtype=torch.float32, device=dev)
        self.heldout = []
        for c2w, t, img in (heldout or []):
            c2w, img = torch.as_tensor(c2w, dtype=torch.float32), torch.as_tensor(img)
            if tuple(c2w.shape) != (3, 4) or tuple(img.shape) != (H, W, 3):
                raise ValueError(f"Scene: a held-out view is (c2w [3,4], t, image [{H},{W},3]), got {list(c2w.shape)} and "
                                 f"{list(img.shape)}")
            img = img.float() / 255 if img.dtype == torch.uint8 else img.float()
            self.heldout.append((c2w.to(dev), float(t), img.to(dev)))
        self._perms = collections.OrderedDict()   # (which, epoch) -> permutation on the device; at most two are kept
        self._tables = L.SceneTablesC(T, H, W, int(self.rgb.dtype == torch.uint8), self.rgb.data_ptr(),
                                      0 if self.disp is None else self.disp.data_ptr(), self.flow_f.data_ptr(),
                                      self.flow_b.data_ptr(), self.masks.data_ptr())

    NPZ_NAMES = ("rgb", "flow_f", "flow_b", "flow_mask_f", "flow_mask_b", "disp", "fg_mask", "poses", "focal")

    @classmethod
    def from_npz(cls, path, device="cuda", seed=20211202):
        """the constructor's arguments under their own names in one .npz; the held-out views as the three arrays
        heldout_c2w [K,3,4], heldout_t [K], heldout_rgb [K,H,W,3]"""
        with np.load(path) as z:
            kw = {n: z[n] for n in cls.NPZ_NAMES if n in z.files}
            if "heldout_c2w" in z.files:
                kw["heldout"] = list(zip(z["heldout_c2w"], z["heldout_t"].tolist(), z["heldout_rgb"]))
        missing = [n for n in cls.NPZ_NAMES[:5] if n not in kw]
        if missing:
            raise ValueError(f"{path}: missing {missing}")
        return cls(device=device, seed=seed, **kw)

    def nbytes(self):
        """device bytes of the per-pixel tables"""
        return sum(t.numel() * t.element_size() for t in (self.rgb, self.disp, self.flow_f, self.flow_b, self.masks)
                   if t is not None)

    # ---- what a trainer needs to know -------------------------------------------------------------------------------
    def bind(self, cfg):
        """T, H, W of `cfg` are the scene's (checked where cfg names them); the focal length is the scene's unless it is
        optimised; without poses there is nothing to hold the poses fixed at"""
        for k in ("T", "H", "W"):
            if cfg.get(k) is not None and int(cfg[k]) != getattr(self, k):
                raise ValueError(f"the config names {k} = {cfg[k]}, the scene has {k} = {getattr(self, k)}")
            cfg[k] = getattr(self, k)
        if not self.has_poses and not cfg.get("optimize_poses", False):
            raise ValueError("the scene has no poses: optimize_poses=False has nothing to hold them at "
                             "(pass poses=, or optimise them)")
        cfg["focal"] = float(self.focal)
        return cfg

    def image(self, frame):
        """training frame `frame` as float [H,W,3] in [0,1]"""
        hw = self.H * self.W
        img = self.rgb[frame * hw: (frame + 1) * hw].view(self.H, self.W, 3)
        return img.float() / 255 if img.dtype == torch.uint8 else img

    # ---- sampler ----------------------------------------------------------------------------------------------------
    def _perm(self, which, epoch):
        key = (int(which), int(epoch))
        p = self._perms.get(key)
        if p is None:
            # host generator seeded with the whole (seed, which, epoch) triple: the same permutation whatever the device,
            # rank or process (the reference draws np.random.permutation, train.py:91)
            g = np.random.default_rng([self.seed, key[0], key[1]])
            p = torch.from_numpy(g.permutation(self.total)).to(self.device)
            self._perms[key] = p
            while len(self._perms) > 2:
                self._perms.popitem(last=False)
        else:
            self._perms.move_to_end(key)
        return p

    def batch(self, it, bs, which=0):
        """batch `it` of sampler `which` (0 | 1): iteration it is batch it % (total // bs) of epoch it // (total // bs)"""
        if which not in (0, 1):
            raise ValueError("which: 0 or 1 (the two independent samplers)")
        if bs <= 0 or self.total < bs:
            raise ValueError(f"a batch of {bs} rays from a scene of {self.total} pixels")
        per_epoch = self.total // bs
        epoch, k = divmod(int(it), per_epoch)
        return self._perm(which, epoch)[k * bs: (k + 1) * bs]

    def ts_of(self, ids):
        return (ids // (self.H * self.W)).float() * (2.0 / (self.T - 1)) - 1.0

    # ---- batch ------------------------------------------------------------------------------------------------------
    def make_batch(self, it, bs, shard=None, ids=None, check=False):
        """SyntheticScene.make_batch: the same keys, shapes, dtypes and values, from one launch.  check=True verifies that
        caller-supplied ids lie in [0, total) (one host sync); out-of-range indices are otherwise undefined."""
        ids, ids2 = (self.batch(it, bs, 0), self.batch(it, bs, 1)) if ids is None else ids
        if shard is not None:
            r, w = shard
            lo, hi = r * bs // w, (r + 1) * bs // w
            ids, ids2 = ids[lo:hi], ids2[lo:hi]
        L.require_device(ids, ids2, self.rgb)
        if ids.dtype != torch.int64 or ids2.dtype != torch.int64 or ids.shape != ids2.shape or ids.dim() != 1:
            raise L.RdrfError("make_batch: ids and ids2 must be int64 vectors of one length")
        if check and ids.numel():
            lo = min(int(ids.min()), int(ids2.min()))
            hi = max(int(ids.max()), int(ids2.max()))
            if lo < 0 or hi >= self.total:
                raise L.RdrfError(f"make_batch: ray indices {lo}..{hi} outside [0, {self.total})")
        ids, ids2 = ids.contiguous(), ids2.contiguous()
        N = ids.shape[0]
        n_al = (N + 63) // 64 * 64    # every output starts on a 256-byte boundary of one buffer
        flat = torch.empty(sum(w for _, w in _BATCH_WIDTHS) * n_al, dtype=torch.float32, device=self.device)
        view = torch.empty(N, dtype=torch.int64, device=self.device)
        o, off = {}, 0
        for name, width in _BATCH_WIDTHS:
            t = flat[off: off + N * width]
            o[name] = t.view(N, width) if width > 1 else t
            off += n_al * width
        assert off == flat.numel()
        out = L.BatchC(*(C.c_void_p(view.data_ptr() if n == "view" else o[n].data_ptr()) for n in L.BATCH_OUTPUTS))
        L.check(L.lib.rdrf_gather_batch(C.byref(self._tables), L.ptr(ids), L.ptr(ids2), N, C.byref(out), L.stream_of(ids)),
                "rdrf_gather_batch")
        return dict(ids=ids, ts=o["ts"], ts_rand=o["ts_rand"], grid=o["grid"], px=o["px"], view=view, rgb=o["rgb"],
                    disp=o["disp"], fg=o["fg"], flow_f=o["flow_f"], flow_b=o["flow_b"], mask_f=o["mask_f"][:, None],
                    mask_b=o["mask_b"][:, None])


@torch.no_grad()
def evaluate(trainer, scene, frames="heldout", alpha_masks=None):
    """PSNR and SSIM of the trainer's fields against the scene's images: frames="heldout" renders the scene's held-out
    cameras through render_view, "train" every training frame through render_frame with the trainer's current poses and
    focal length (the per-image body of renderer.py:661-966 `evaluation`).  Everything stays on the device until one
    transfer at the end.  `alpha_masks`: as render_rays (True: the fields' own alphaMask; the masked render).
    Returns dict(psnr=[...], ssim=[...], psnr_mean, ssim_mean)."""
    c = trainer.cfg
    st, dy, H, W, S, rt = trainer.st, trainer.dy, scene.H, scene.W, c["n_samples"], c["ray_type"]
    focal = trainer.focal()
    focal = focal.detach() if torch.is_tensor(focal) else focal
    pairs = []
    if frames == "heldout":
        if not scene.heldout:
            raise ValueError("evaluate: the scene has no held-out views")
        for c2w, t, img in scene.heldout:
            rgb, _ = render_view(st, dy, c2w, focal, H, W, t, N_samples=S, ray_type=rt, maps=False, alpha_masks=alpha_masks)
            pairs.append((rgb, img))
    elif frames == "train":
        poses = trainer.pose_table().detach()
        for f in range(scene.T):
            rgb, _ = render_frame(st, dy, poses, focal, f, H, W, N_samples=S, ray_type=rt, alpha_masks=alpha_masks)
            pairs.append((rgb, scene.image(f)))
    else:
        raise ValueError('evaluate: frames is "heldout" or "train"')
    vals = torch.stack([torch.stack([psnr(a, b).double(), ssim(a, b)]) for a, b in pairs]).cpu()   # the one sync
    ps, ss = vals[:, 0].tolist(), vals[:, 1].tolist()
    return dict(psnr=ps, ssim=ss, psnr_mean=sum(ps) / len(ps), ssim_mean=sum(ss) / len(ss))
