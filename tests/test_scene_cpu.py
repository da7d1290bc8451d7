"""Array-backed training set (scene.Scene) and the resolution schedule, as far as they run without a GPU: the schedule
functions against the stage tables of scene_config, the sampler's SimpleSampler semantics (train.py:81-93) as a pure
function, the constructor's validation, the pose packing and the boundary (header, version)."""
import os
import re

import numpy as np
import pytest
import torch

from _util import pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def arrays(T=3, H=5, W=7, seed=0, rgb_dtype=np.uint8, poses=True):
    r = np.random.default_rng(seed)
    a = dict(rgb=r.integers(0, 256, (T, H, W, 3)).astype(np.uint8), flow_f=r.normal(size=(T, H, W, 2)).astype(np.float32),
             flow_b=r.normal(size=(T, H, W, 2)).astype(np.float32), flow_mask_f=r.random((T, H, W)) < 0.8,
             flow_mask_b=r.random((T, H, W)) < 0.8, disp=r.random((T, H, W)).astype(np.float32),
             fg_mask=r.random((T, H, W)) < 0.2)
    if rgb_dtype != np.uint8:
        a["rgb"] = (a["rgb"].astype(np.float32) / np.float32(255)).astype(np.float32)
    if poses:
        a["poses"] = r.normal(size=(T, 3, 4)).astype(np.float32)
    return a


# ---- schedule ------------------------------------------------------------------------------------------------------
def test_resolution_stages_reproduce_the_stage_tables():
    import rodynrf
    st = rodynrf.resolution_stages(rodynrf.scene_config("nvidia"))
    assert [s[1] for s in st] == [[141, 157, 94], [174, 194, 116], [216, 240, 144], [267, 298, 178], [331, 368, 220]]
    assert [s[2] for s in st] == [115, 142, 176, 218, 270]
    assert [s[0] for s in st] == [0, 8001, 12001, 16001, 22001]   # the grid changes after the step of upsamp_list[k]
    for k, stage in enumerate(("stage0", "up1", "up2", "up3", "final")):
        c = rodynrf.scene_config("nvidia", stage)
        assert (c["grid"], c["n_samples"]) == (st[k][1], st[k][2])
    st = rodynrf.resolution_stages(rodynrf.scene_config("nvidia_no_poses"))
    assert len(st) == 8 and st[0][1:] == ([17, 19, 11], 13) and st[-1][1:] == ([706, 786, 471], 578)
    c = rodynrf.scene_config("nvidia_no_poses", "final")
    assert (c["grid"], c["n_samples"]) == st[-1][1:]
    st = rodynrf.resolution_stages(rodynrf.scene_config("davis"))
    assert len(st) == 8 and st[0][1:] == ([16, 16, 16], 13) and st[-1][1:] == ([256, 256, 256], 221)


def test_schedule_functions_and_the_sample_cap():
    import rodynrf
    aabb = [[-1.5, -1.67, -1.0], [1.5, 1.67, 1.0]]
    assert rodynrf.N_to_reso(128 ** 3, aabb) == [141, 157, 94]
    assert rodynrf.N_to_reso(16 ** 3, torch.tensor([[-2.0] * 3, [2.0] * 3])) == [16, 16, 16]
    assert rodynrf.cal_n_samples([141, 157, 94], 2.0) == 115 and rodynrf.cal_n_samples([3, 4, 0], 0.5) == 10
    cfg = dict(rodynrf.scene_config("nvidia"), nSamples=150)
    assert [s[2] for s in rodynrf.resolution_stages(cfg)] == [115, 142, 150, 150, 150]


# ---- sampler -------------------------------------------------------------------------------------------------------
def test_sampler_epochs_are_disjoint_permutations_and_batch_is_pure():
    import rodynrf
    sc = rodynrf.Scene(**arrays(), device="cpu", seed=5)
    total, bs = sc.total, 16          # 105 pixels: 6 batches per epoch, a tail of 9 dropped
    per = total // bs
    assert (total, per) == (105, 6)
    for which in (0, 1):
        for epoch in (0, 1, 3):
            ids = torch.cat([sc.batch(epoch * per + k, bs, which) for k in range(per)])
            assert ids.dtype == torch.int64 and ids.numel() == per * bs
            assert int(ids.min()) >= 0 and int(ids.max()) < total and ids.unique().numel() == per * bs
    # pure: any order, any repetition, a second object with the same seed
    sc2 = rodynrf.Scene(**arrays(), device="cpu", seed=5)
    order = [(13, 1), (0, 0), (7, 0), (13, 1), (2, 1), (0, 0), (40, 0), (7, 0)]
    first = {}
    for it, which in order:
        ids = sc.batch(it, bs, which).clone()
        assert torch.equal(first.setdefault((it, which), ids), ids)
        assert len(sc._perms) <= 2      # at most two epochs' permutations are kept
    for (it, which), ids in first.items():
        assert torch.equal(sc2.batch(it, bs, which), ids)
    assert not torch.equal(sc.batch(3, bs, 0), sc.batch(3, bs, 1))            # the two samplers are independent
    assert not torch.equal(sc.batch(3, bs, 0), sc.batch(3 + per, bs, 0))      # consecutive epochs differ
    assert not torch.equal(sc.batch(3, bs, 0), rodynrf.Scene(**arrays(), device="cpu", seed=6).batch(3, bs, 0))
    # another batch size is another cut of the same epoch permutation
    assert torch.equal(torch.cat([sc.batch(0, 8, 0), sc.batch(1, 8, 0)]), sc.batch(0, 16, 0))
    with pytest.raises(ValueError):
        sc.batch(0, total + 1, 0)
    assert sc.batch(0, total, 0).numel() == total
    with pytest.raises(ValueError):
        sc.batch(0, bs, 2)


def test_ts_of_matches_the_table_expression():
    import rodynrf
    sc = rodynrf.Scene(**arrays(T=7), device="cpu")
    ids = torch.arange(sc.total)
    table = ((ids // (5 * 7)).float() * (2.0 / (7 - 1)) - 1.0)
    assert torch.equal(sc.ts_of(ids), table) and float(table[0]) == -1.0 and float(table[-1]) == 1.0


# ---- constructor ---------------------------------------------------------------------------------------------------
def test_constructor_validation():
    import rodynrf
    a = arrays()
    for name, bad in (("flow_f", a["flow_f"][:, :, :-1]), ("flow_b", a["flow_b"][:-1]), ("flow_mask_f", a["flow_mask_f"][:, :-1]),
                      ("flow_mask_b", a["flow_mask_b"][..., None].repeat(2, -1)), ("disp", a["disp"][:, :, 1:]),
                      ("fg_mask", a["fg_mask"][1:]), ("poses", a["poses"][:-1]), ("poses", a["poses"][:, :, :3]),
                      ("rgb", a["rgb"][..., :2]), ("rgb", a["rgb"].astype(np.float64)), ("rgb", a["rgb"][:1])):
        with pytest.raises(ValueError):
            rodynrf.Scene(**dict(a, **{name: bad}), device="cpu")
    for name in ("flow_f", "flow_b", "flow_mask_f", "flow_mask_b"):   # a missing flow or flow mask
        with pytest.raises(ValueError):
            rodynrf.Scene(**dict(a, **{name: None}), device="cpu")
    with pytest.raises(ValueError):
        rodynrf.Scene(**a, heldout=[(np.eye(4, dtype=np.float32), 0.0, a["rgb"][0])], device="cpu")
    sc = rodynrf.Scene(**a, heldout=[(np.eye(3, 4, dtype=np.float32), 0.5, a["rgb"][0])], device="cpu")
    assert sc.heldout[0][2].dtype == torch.float32 and float(sc.heldout[0][2].max()) <= 1.0
    # T, H, W of a config are the scene's; a config that names others is refused
    cfg = sc.bind(dict(optimize_poses=False))
    assert (cfg["T"], cfg["H"], cfg["W"]) == (3, 5, 7) and cfg["focal"] == pytest.approx(3.5 * 3 ** 0.5)
    with pytest.raises(ValueError):
        sc.bind(dict(T=3, H=5, W=8))
    # without poses: the identity initialisation, and nothing to hold them fixed at
    a.pop("poses")
    sp = rodynrf.Scene(**a, device="cpu")
    ident = torch.zeros(3, 9)
    ident[:, 0] = 1.0
    ident[:, 4] = 1.0
    assert torch.equal(sp.poses, ident)
    with pytest.raises(ValueError):
        sp.bind(dict(optimize_poses=False))
    assert sp.bind(dict(optimize_poses=True))["T"] == 3


def test_storage_is_compact():
    import rodynrf
    a = arrays()
    sc = rodynrf.Scene(**a, device="cpu")
    assert sc.rgb.dtype == torch.uint8 and sc.masks.dtype == torch.uint8 and sc.masks.shape == (sc.total,)
    m = sc.masks.numpy()
    assert np.array_equal(m & 1, a["fg_mask"].reshape(-1)) and np.array_equal((m >> 1) & 1, a["flow_mask_f"].reshape(-1))
    assert np.array_equal((m >> 2) & 1, a["flow_mask_b"].reshape(-1))
    # 3 + 1 + 4 + 8 + 8 bytes per pixel; no pixel-centre, integer-pixel, view or time table
    assert sc.nbytes() == sc.total * 24
    assert not any(hasattr(sc, n) for n in ("grid_table", "px_table", "view_table", "ts_table"))
    # the mask conventions: integer non-zero, float >= 0.5
    s2 = rodynrf.Scene(**dict(a, fg_mask=a["fg_mask"].astype(np.uint8) * 255, flow_mask_f=a["flow_mask_f"].astype(np.float32)),
                       device="cpu")
    assert torch.equal(s2.masks, sc.masks)
    assert rodynrf.Scene(**arrays(rgb_dtype=np.float32), device="cpu").rgb.dtype == torch.float32


def test_pose_packing_is_columns_0_1_3():
    import rodynrf
    c2w = torch.arange(2 * 12, dtype=torch.float32).view(2, 3, 4)
    p9 = rodynrf.pack_poses(c2w)
    assert p9.shape == (2, 9)
    assert torch.equal(p9[:, 0:3], c2w[:, :, 0]) and torch.equal(p9[:, 3:6], c2w[:, :, 1]) and torch.equal(p9[:, 6:9], c2w[:, :, 3])
    assert torch.equal(rodynrf.Scene(**dict(arrays(T=2), poses=c2w.numpy()), device="cpu").poses, p9)
    # an orthonormal camera survives the round trip through the trainer's pose_to_mtx
    q, _ = torch.linalg.qr(torch.randn(3, 3, generator=torch.Generator().manual_seed(0)))
    q = q * torch.sign(torch.linalg.det(q))
    m = torch.cat([q, torch.tensor([[0.1], [0.2], [0.3]])], 1)[None]
    assert torch.allclose(rodynrf.pose_to_mtx(rodynrf.pack_poses(m)), m, atol=1e-6)


def test_from_npz(tmp_path):
    import rodynrf
    a = arrays()
    path = str(tmp_path / "scene.npz")
    np.savez(path, focal=np.float32(40.0), heldout_c2w=np.eye(3, 4, dtype=np.float32)[None], heldout_t=np.array([0.25]),
             heldout_rgb=a["rgb"][:1], **a)
    sc = rodynrf.Scene.from_npz(path, device="cpu", seed=3)
    ref = rodynrf.Scene(**a, focal=40.0, device="cpu", seed=3)
    for n in ("rgb", "disp", "flow_f", "flow_b", "masks", "poses", "focal"):
        assert torch.equal(getattr(sc, n), getattr(ref, n)), n
    assert len(sc.heldout) == 1 and sc.heldout[0][1] == 0.25 and torch.equal(sc.batch(2, 16, 1), ref.batch(2, 16, 1))
    np.savez(path, rgb=a["rgb"], flow_f=a["flow_f"])
    with pytest.raises(ValueError):
        rodynrf.Scene.from_npz(path, device="cpu")


def test_make_batch_refuses_host_tables():
    import rodynrf
    sc = rodynrf.Scene(**arrays(), device="cpu")
    with pytest.raises(rodynrf.RdrfError):
        sc.make_batch(0, 16)


# ---- boundary ------------------------------------------------------------------------------------------------------
def test_header_declares_the_gather_and_the_version_stays_6():
    L = pkg()
    hdr = open(os.path.join(ROOT, "include", "rodynrf.h")).read()
    assert re.search(r"\bint\s+rdrf_gather_batch\s*\(\s*const\s+RdrfSceneTables\s*\*", hdr)
    assert "} RdrfSceneTables;" in hdr and "} RdrfBatch;" in hdr
    assert re.search(r"#define\s+RDRF_ABI_VERSION\s+6\b", hdr) and L.ABI_VERSION == 6 and L.lib.rdrf_abi_version() == 6
    assert "rdrf_gather_batch" in L.SYMBOLS and hasattr(L.lib, "rdrf_gather_batch")
    # the binding's structs follow the header's field order
    for struct, cls in (("RdrfSceneTables", L.SceneTablesC), ("RdrfBatch", L.BatchC)):
        body = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct + ";", hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [n for decl in body.split(";") for n in re.findall(r"\*?\s*(\w+)\s*(?:,|$)", decl.strip())]
        assert names == [f[0] for f in cls._fields_], (struct, names)
