"""GPU tests of the mesh simplification (csrc/rdrf_simplify.hip, mesh.simplify_mesh) against the numpy restatement of
tests/_simplify_prim.py: bit-equal counts, remap, faces, colours and positions on dyadic inputs at every size where the loop
structure changes, bounds counted from the kernels' operations on general inputs, the properties of a clustered real mesh,
isolation (poisoned workspace, guarded outputs, untouched inputs) and determinism (two runs, the deterministic twin)."""
import ctypes as C

import numpy as np
import pytest
import torch

import _iso_prim as P
import _simplify_prim as S
from _twin import CHILD, run_twin
from _util import pkg, record_margin

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 5   # poisoned rows in front of every output


def sort_tile():
    L = pkg()
    out = (C.c_ulong * 9)()
    assert L.lib.rdrf_selftest_sort_describe(1, 100000, 18, out, 9) == 9
    return int(out[4])


def run(verts, faces, origin, cell, n, normals=None, colors=None, drop=True, ws_byte=0xFF):
    """the two native calls on numpy inputs with a poisoned workspace of exactly the advertised size and guarded, oversized
    outputs; checks that nothing outside [0, nv) / [0, nf) was written and that the inputs are unchanged"""
    L = pkg()
    v_np = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    f_np = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
    V, F = len(v_np), len(f_np)
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    v, f, nr, co = dev(v_np), dev(f_np), dev(normals), dev(colors)
    o3, c3, n3 = (C.c_float * 3)(*[float(x) for x in origin]), (C.c_float * 3)(*[float(x) for x in cell]), (C.c_int * 3)(*[int(x) for x in n])
    nbytes = L.lib.rdrf_simplify_ws_bytes(V, F, n3)
    assert nbytes > 0 and nbytes % 256 == 0
    ws = torch.full((nbytes,), ws_byte, dtype=torch.uint8, device=DEV)
    counts = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    remap = torch.full((V + 2 * GUARD,), -77, dtype=torch.int32, device=DEV)
    s = L.stream_of(ws)
    L.check(L.lib.rdrf_simplify_count(L.ptr(v), V, L.ptr(f), F, o3, c3, n3, int(drop), L.ptr(ws), nbytes, L.ptr(counts),
                                      C.c_void_p(remap.data_ptr() + 4 * GUARD), s), "rdrf_simplify_count")
    nv, nf = (int(x) for x in counts.cpu().tolist())
    assert 0 <= nv <= V and 0 <= nf <= F
    vo = torch.full((V + 2 * GUARD, 3), -5.0e8, dtype=torch.float32, device=DEV)
    fo = torch.full((F + 2 * GUARD, 3), -99, dtype=torch.int32, device=DEV)
    no = None if normals is None else torch.full((V + 2 * GUARD, 3), -5.0e8, dtype=torch.float32, device=DEV)
    cout = None if colors is None else torch.full((V + 2 * GUARD, 3), 0xA5, dtype=torch.uint8, device=DEV)
    at = lambda t, item: None if t is None else C.c_void_p(t.data_ptr() + GUARD * 3 * item)
    L.check(L.lib.rdrf_simplify_emit(L.ptr(v), L.ptr(nr), L.ptr(co), V, L.ptr(f), F, L.ptr(ws), at(vo, 4), at(no, 4), at(cout, 1), at(fo, 4),
                                     nv, nf, s), "rdrf_simplify_emit")
    torch.cuda.synchronize()
    out = {"counts": (nv, nf)}
    rm = remap.cpu().numpy()
    assert (rm[:GUARD] == -77).all() and (rm[GUARD + V:] == -77).all()
    out["remap"] = rm[GUARD:GUARD + V] if V and F else np.full(V, -1, np.int32)   # V = 0 or F = 0 writes the counts only
    if not (V and F):
        assert (rm == -77).all()
    for name, t, rows, poison in (("verts", vo, nv, np.float32(-5.0e8)), ("faces", fo, nf, -99), ("normals", no, nv, np.float32(-5.0e8)),
                                  ("colors", cout, nv, 0xA5)):
        if t is None:
            continue
        a = t.cpu().numpy()
        assert (a[:GUARD] == poison).all() and (a[GUARD + rows:] == poison).all(), f"{name}: written outside its {rows} rows"
        out[name] = a[GUARD:GUARD + rows]
    assert v.cpu().numpy().tobytes() == v_np.tobytes() and f.cpu().numpy().tobytes() == f_np.tobytes()
    if normals is not None:
        assert nr.cpu().numpy().tobytes() == np.ascontiguousarray(normals).tobytes()
    if colors is not None:
        assert co.cpu().numpy().tobytes() == np.ascontiguousarray(colors).tobytes()
    return out


def assert_exact(got, ref, what):
    assert got["counts"] == ref["counts"], (what, got["counts"], ref["counts"])
    assert np.array_equal(got["remap"], ref["remap"]), what
    assert np.array_equal(got["faces"], ref["faces"]), what
    assert got["verts"].tobytes() == ref["verts"].tobytes(), what
    if "colors" in ref:
        assert np.array_equal(got["colors"], ref["colors"]), what


# ---- exact cases: dyadic coordinates (multiples of 2^-6 below 2^8), so every fp64 sum is exact whatever its order ------------
N64 = (64, 64, 64)          # cells of 1/8 from the origin: 18 key bits, two sort passes
CELL = (0.125, 0.125, 0.125)


def dyadic_case(rng, V, regime, n=N64):
    """vertices of the regime on the lattice n of 1/8 cells; faces: 2 V + 3 random triples"""
    ncell = n[0] * n[1] * n[2]
    if regime == "own":            # every vertex in a cell of its own (an odd stride is a bijection of 2^18)
        assert V <= ncell and ncell % 2 == 0
        cell_of = (np.arange(V, dtype=np.int64) * 104729 + 12345) % ncell
    elif regime == "one":          # all in one cell
        cell_of = np.full(V, (5 * n[1] + 6) * n[2] + 7, dtype=np.int64) % ncell
    else:                          # a third as many occupied cells as vertices, empty cells between them
        m = min(max(1, V // 3), ncell)
        pool = rng.choice(ncell, size=m, replace=False) if ncell < 2 ** 24 else rng.integers(0, ncell, m)
        cell_of = pool[rng.integers(0, len(pool), V)].astype(np.int64)
    c = np.stack((cell_of // (n[1] * n[2]), (cell_of // n[2]) % n[1], cell_of % n[2]), 1)
    verts = (c * 8 + rng.integers(0, 8, (V, 3))) / 64.0
    assert np.abs(verts).max() < 256 if V else True
    faces = rng.integers(0, max(V, 1), (2 * V + 3, 3))
    colors = rng.integers(0, 256, (V, 3)).astype(np.uint8)
    return verts.astype(np.float32), faces.astype(np.int32), colors


def exact_sizes():
    try:
        tile = sort_tile()
    except Exception:   # collection without the library: the test itself fails, not the collection
        tile = 2048
    return sorted({1, 2, 255, 256, 257, tile - 1, tile, tile + 1, 65535, 65536, 65537})


@pytest.mark.parametrize("V", exact_sizes())
def test_exact_on_dyadic_inputs(V):
    tile = sort_tile()
    assert {tile - 1, tile, tile + 1} <= set(exact_sizes())          # the sizes around the sort's tile are among the cases
    rng = np.random.default_rng(V)
    for regime in ("own", "one", "random"):
        verts, faces, colors = dyadic_case(rng, V, regime)
        for drop in (True, False):
            ref = S.simplify(verts, faces, (0, 0, 0), CELL, N64, colors=colors, drop_unreferenced=drop)
            got = run(verts, faces, (0, 0, 0), CELL, N64, colors=colors, drop=drop)
            assert_exact(got, ref, (V, regime, drop))
        if regime == "own" and V >= 255:
            assert ref["counts"][0] == V and ref["counts"][1] > V        # nothing merges
        if regime == "one":
            assert ref["counts"] == (1, 0)                               # (drop off: the one cluster stays)


@pytest.mark.parametrize("n,bits", [((1, 1, 1), 0), ((1290, 1290, 1290), 31)])
def test_exact_at_the_narrowest_and_the_widest_key(n, bits):
    assert (n[0] * n[1] * n[2] - 1).bit_length() == bits and n[0] * n[1] * n[2] < 2 ** 31
    rng = np.random.default_rng(bits)
    V = 3001
    verts, faces, colors = dyadic_case(rng, V, "random", n)       # 1290 / 8 = 161.25 < 2^8
    for drop in (True, False):
        ref = S.simplify(verts, faces, (0, 0, 0), CELL, n, colors=colors, drop_unreferenced=drop)
        got = run(verts, faces, (0, 0, 0), CELL, n, colors=colors, drop=drop)
        assert_exact(got, ref, (n, drop))
    assert ref["counts"] == ((1, 0) if bits == 0 else ref["counts"]) and (bits == 0 or 900 < ref["counts"][0] <= 1000)


@pytest.mark.parametrize("drop", [True, False])
def test_no_faces_and_no_vertices(drop):
    rng = np.random.default_rng(5)
    verts, _, colors = dyadic_case(rng, 300, "random")
    for v, f, c in ((verts, np.zeros((0, 3), np.int32), colors), (verts[:0], np.zeros((0, 3), np.int32), colors[:0])):
        got = run(v, f, (0, 0, 0), CELL, N64, colors=c, drop=drop)
        assert got["counts"] == (0, 0) and len(got["verts"]) == 0 and len(got["faces"]) == 0
        assert_exact(got, S.simplify(v, f, (0, 0, 0), CELL, N64, colors=c, drop_unreferenced=drop), len(v))


# ---- general inputs ----------------------------------------------------------------------------------------------------------
GEN_SEED, GEN_V, GEN_F = 2024, 50000, 120000
GEN_ORIGIN, GEN_CELL, GEN_N = (-1.03, -0.77, 0.41), (0.137, 0.21, 0.173), (15, 8, 12)


def general_case():
    rng = np.random.default_rng(GEN_SEED)
    lo, ext = np.array(GEN_ORIGIN), np.array(GEN_CELL) * np.array(GEN_N)
    verts = (lo - 0.05 * ext + rng.random((GEN_V, 3)) * 1.1 * ext).astype(np.float32)    # some fall outside and clamp
    faces = rng.integers(0, GEN_V, (GEN_F, 3)).astype(np.int32)
    normals = rng.standard_normal((GEN_V, 3)).astype(np.float32)
    normals /= np.linalg.norm(normals, axis=1, keepdims=True).astype(np.float32)
    colors = rng.integers(0, 256, (GEN_V, 3)).astype(np.uint8)
    return verts, faces, normals, colors


def near_a_boundary(verts):
    """vertices with a coordinate within one fp32 rounding of a cell boundary: where t = (v - origin) / cell in exact
    arithmetic lies within the two roundings of its fp32 evaluation (2^-23 |t| + the subtraction's 2^-24 |v - o| / cell) of a
    whole number"""
    v = verts.astype(np.float64)
    o, c = np.float32(GEN_ORIGIN).astype(np.float64), np.float32(GEN_CELL).astype(np.float64)
    t = (v - o) / c
    slack = 2.0 ** -23 * np.abs(t) + 2.0 ** -24 * (np.abs(v) + np.abs(o)) / c
    return (np.abs(t - np.rint(t)) <= slack).any(1)


def test_general_inputs():
    verts, faces, normals, colors = general_case()
    left_out = int(near_a_boundary(verts).sum())
    print(f"{left_out} of {GEN_V} vertices lie within one fp32 rounding of a cell boundary")
    assert left_out <= GEN_V // 100
    ref = S.simplify(verts, faces, GEN_ORIGIN, GEN_CELL, GEN_N, normals=normals, colors=colors)
    got = run(verts, faces, GEN_ORIGIN, GEN_CELL, GEN_N, normals=normals, colors=colors)
    # topology: the restatement forms t with the same two fp32 roundings, so no vertex has to be left out at all; a mismatch
    # is reported with the number of mismatching vertices outside the boundary set
    bad = got["remap"] != ref["remap"]
    assert not bad.any(), f"{int(bad.sum())} vertices differ, {int((bad & ~near_a_boundary(verts)).sum())} of them away from every boundary"
    assert got["counts"] == ref["counts"] and np.array_equal(got["faces"], ref["faces"]) and np.array_equal(got["colors"], ref["colors"])
    assert 1000 < ref["counts"][0] <= 15 * 8 * 12 and ref["k"].max() > 20
    # positions: one fp32 rounding + k fp64 additions
    k = ref["k"][:, None].astype(np.float64)
    bound = 2.0 ** -24 * np.abs(ref["mean"]) + k * 2.0 ** -53 * ref["abs_sum"]
    err = np.abs(got["verts"].astype(np.float64) - ref["mean"])
    ratio = float((err / bound).max())
    record_margin("simplify.position", ratio)
    assert ratio <= 1.0, ratio
    # normals, counted from k_simp_verts: k additions per component (k 2^-53 sum|n_d| each), then one division by the largest
    # component, three products and two additions, a square root and a division (8 roundings of values <= sqrt(3) in fp64),
    # relative to the length of the sum where it cancels, then one rounding to fp32 of a value <= 1; twice, because the
    # restatement carries the same roundings
    length = np.linalg.norm(ref["nsum"], axis=1, keepdims=True)
    assert (length > 0).all()
    nbound = 2.0 * (2.0 ** -24 + 2.0 ** -53 * (8.0 * np.sqrt(3.0) + 2.0 * k * ref["nabs"].sum(1, keepdims=True) / length))
    nerr = np.abs(got["normals"].astype(np.float64) - ref["normals"].astype(np.float64))
    nratio = float((nerr / nbound).max())
    record_margin("simplify.normal", nratio)
    assert nratio <= 1.0, nratio
    unit = np.abs(np.linalg.norm(got["normals"].astype(np.float64), axis=1) - 1.0).max()
    record_margin("simplify.normal_length", float(unit / (3 * 2.0 ** -24)))
    assert unit <= 3 * 2.0 ** -24, unit


# ---- a real mesh -------------------------------------------------------------------------------------------------------------
def ball_mesh():
    import rodynrf
    vol = P.sphere_volume(P.SHAPE, P.AABB, (0.03, -0.12, 0.21), 1.0).astype(np.float32)     # reaches the box: cap closes it
    assert (vol[0] > 0).any() or (vol[:, 0] > 0).any() or (vol[:, :, 0] > 0).any() or (vol[-1] > 0).any()
    out = rodynrf.extract_isosurface(torch.from_numpy(vol).to(DEV), 0.0, torch.from_numpy(P.AABB), cap=True, normals=True)
    return vol, out


@pytest.mark.parametrize("K", [2, 3])
def test_a_capped_ball(K, tmp_path):
    import rodynrf
    vol, (v, f, nrm) = ball_mesh()
    assert S.unbalanced_edges(f.cpu().numpy()) == 0
    lat = rodynrf.simplify_lattice(P.AABB, P.SHAPE, K, cap=True)
    sv, sf, sn, remap = rodynrf.simplify_mesh(v, f, normals=nrm, return_remap=True, **lat)
    direct = rodynrf.extract_isosurface(torch.from_numpy(vol).to(DEV), 0.0, torch.from_numpy(P.AABB), cap=True, normals=True, simplify=K)
    for a, b in zip((sv, sf, sn), direct):
        assert a.dtype == b.dtype and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    origin, cell, n = S.lattice(P.AABB, P.SHAPE, K, cap=True)
    ref = S.simplify(v.cpu().numpy(), f.cpu().numpy(), origin, cell, n, normals=nrm.cpu().numpy())
    faces, verts = sf.cpu().numpy(), sv.cpu().numpy()
    assert np.array_equal(faces, ref["faces"]) and np.array_equal(remap.cpu().numpy(), ref["remap"])
    assert 0 < len(verts) < len(v) and 0 < len(faces) < len(f)
    print(f"K={K}: {len(v)} -> {len(verts)} vertices, {len(f)} -> {len(faces)} faces")
    assert S.unbalanced_edges(faces) == 0
    assert (faces[:, 0] != faces[:, 1]).all() and (faces[:, 1] != faces[:, 2]).all() and (faces[:, 0] != faces[:, 2]).all()
    assert np.array_equal(np.unique(faces), np.arange(len(verts)))
    # every output vertex lies in the closed box of its members' cell, widened by one ulp
    c = np.zeros((len(verts), 3), dtype=np.int64)
    c[ref["remap"][ref["remap"] >= 0]] = S.cells(v.cpu().numpy(), origin, cell, n)[ref["remap"] >= 0]
    o64, c64 = origin.astype(np.float64), cell.astype(np.float64)
    lo, hi = o64 + c * c64, o64 + (c + 1) * c64
    # in the fp32 lattice coordinates that define the cells, no widening is needed: the mean lies between its members
    assert np.array_equal(S.cells(verts, origin, cell, n), c)
    # in world coordinates the cell's faces are where t = (v - origin) / cell crosses a whole number in EXACT arithmetic, and
    # the kernel's t carries two fp32 roundings: the box is widened by one fp32 ulp relative to the lattice origin,
    # 2^-23 |face - origin| (an ulp of |face| alone is too little wherever the origin is far from zero: at x = 1 with the
    # origin at -1.09 the two roundings move a face by 2.1 * 2^-23, and the ulp of 1 is 2^-23)
    eps = float(np.finfo(np.float32).eps) * (1.0 + 2.0 ** -20)
    assert (verts >= lo - eps * np.abs(lo - o64)).all() and (verts <= hi + eps * np.abs(hi - o64)).all()
    assert np.abs(np.linalg.norm(sn.cpu().numpy().astype(np.float64), axis=1) - 1.0).max() <= 3 * 2.0 ** -24
    path = str(tmp_path / "ball.ply")
    rodynrf.write_ply(path, sv, sf, normals=sn)
    back = rodynrf.read_ply(path)
    assert back["verts"].tobytes() == verts.tobytes() and np.array_equal(back["faces"], faces)
    assert back["normals"].tobytes() == sn.cpu().numpy().tobytes() and back["colors"] is None


def test_field_meshes_equal_simplify_mesh_of_the_unsimplified_call(tmp_path):
    import rodynrf
    from test_gpu_iso import LATTICE, fixture_fields, mid_level
    fields = fixture_fields()
    grid = list(LATTICE)
    for field, t in ((fields["static"], None), (fields["dynamic"], 0.25)):
        alpha, level = mid_level(field, [0.0 if t is None else t])
        lat = rodynrf.simplify_lattice(field.aabb, alpha.shape, 2)
        plain = rodynrf.field_mesh(field, t, level, grid, normals=True)
        assert plain[0].shape[0] > 0 and plain[1].shape[0] > 0
        want = rodynrf.simplify_mesh(plain[0], plain[1], normals=plain[2], **lat)
        got = rodynrf.field_mesh(field, t, level, grid, normals=True, simplify=2)
        assert len(got) == 3 and got[0].shape[0] <= plain[0].shape[0]
        for a, b in zip(got, want):
            assert a.dtype == b.dtype and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
        seq = list(rodynrf.mesh_sequence(field, [0.0 if t is None else t], level, grid, normals=True, simplify=2))
        assert all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() for a, b in zip(seq[0], want))
        cplain = rodynrf.colored_mesh(field, t, level, grid)
        want = rodynrf.simplify_mesh(cplain[0], cplain[1], colors=cplain[2], **lat)
        got = rodynrf.colored_mesh(field, t, level, grid, simplify=2)
        assert len(got) == 3 and got[2].dtype == torch.uint8
        for a, b in zip(got, want):
            assert a.dtype == b.dtype and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
        path = str(tmp_path / "field.ply")
        out = field.export_mesh(path, t, level, gridSize=grid, color_view=(0, 0, 1), simplify=2)
        back = rodynrf.read_ply(path)
        assert back["verts"].tobytes() == want[0].cpu().numpy().tobytes() and np.array_equal(back["faces"], want[1].cpu().numpy())
        assert np.array_equal(back["colors"], want[2].cpu().numpy()) and len(out) == 3


def test_python_surface_lattices_and_refusals():
    import rodynrf
    rng = np.random.default_rng(3)
    verts, faces, colors = dyadic_case(rng, 500, "random")
    v, f = torch.from_numpy(verts).to(DEV), torch.from_numpy(faces).to(DEV)
    ref = S.simplify(verts, faces, (0, 0, 0), CELL, N64)
    box = [0, 0, 0, 8, 8, 8]
    for kw in (dict(cell=0.125, aabb=box), dict(cell=CELL, aabb=box), dict(grid=N64, aabb=box), dict(cell=CELL, grid=N64, aabb=box)):
        out = rodynrf.simplify_mesh(v, f, **kw)
        assert len(out) == 2 and out[0].cpu().numpy().tobytes() == ref["verts"].tobytes() and np.array_equal(out[1].cpu().numpy(), ref["faces"])
    # aabb=None: the box of the vertices
    lo, hi = verts.min(0), verts.max(0)
    n = [max(1, int(np.ceil((float(hi[d]) - float(lo[d])) / 0.5))) for d in range(3)]
    ref = S.simplify(verts, faces, lo, (0.5, 0.5, 0.5), n, colors=colors, drop_unreferenced=False)
    out = rodynrf.simplify_mesh(v, f, cell=0.5, colors=torch.from_numpy(colors).to(DEV), drop_unreferenced=False, return_remap=True)
    assert len(out) == 4 and out[0].cpu().numpy().tobytes() == ref["verts"].tobytes() and np.array_equal(out[1].cpu().numpy(), ref["faces"])
    assert np.array_equal(out[2].cpu().numpy(), ref["colors"]) and np.array_equal(out[3].cpu().numpy(), ref["remap"])
    for bad in (dict(verts=v.double()), dict(verts=v[:, :2]), dict(faces=f.long()), dict(normals=v[:3]), dict(colors=v), dict(cell=None),
                dict(cell=(1, 2)), dict(cell=0.0), dict(grid=(2, 2)), dict(cell=None, grid=(0, 2, 2))):
        kw = dict(verts=v, faces=f, cell=0.5)
        kw.update(bad)
        with pytest.raises(rodynrf.RdrfError, match="simplify_mesh"):
            rodynrf.simplify_mesh(**kw)


# ---- determinism -------------------------------------------------------------------------------------------------------------
def det_case():
    """what both libraries run (tests/_det_child.py case)"""
    out = {}
    verts, faces, normals, colors = general_case()
    for byte in (0xFF, 0x00):
        got = run(verts[:20000], faces[:50000] % 20000, GEN_ORIGIN, GEN_CELL, GEN_N, normals=normals[:20000], colors=colors[:20000], ws_byte=byte)
        for k in ("verts", "faces", "normals", "colors", "remap"):
            out[f"general{byte}.{k}"] = torch.from_numpy(np.ascontiguousarray(got[k]))
    rng = np.random.default_rng(9)
    v, f, c = dyadic_case(rng, 4099, "random")
    got = run(v, f, (0, 0, 0), CELL, N64, colors=c, drop=False)
    for k in ("verts", "faces", "colors", "remap"):
        out[f"dyadic.{k}"] = torch.from_numpy(np.ascontiguousarray(got[k]))
    return out


def test_two_runs_and_both_workspace_poisons_give_the_same_bits():
    first, again = det_case(), det_case()
    for k in first:
        assert first[k].numpy().tobytes() == again[k].numpy().tobytes(), k
    for k in [k for k in first if k.startswith("general255.")]:
        assert first[k].numpy().tobytes() == first[k.replace("general255.", "general0.")].numpy().tobytes(), k


def test_deterministic_library_gives_the_same_bits(tmp_path):
    mine = det_case()
    det = run_twin(tmp_path, [CHILD, "case", "test_gpu_simplify"], det=True)
    assert set(det) == set(mine)
    for k, v in mine.items():
        assert v.numpy().tobytes() == det[k].numpy().tobytes(), k
