"""The gradient scatter family and the radix sort on their own (rdrf_selftest_scatter: the product's launch functions on data the
test supplies; rdrf_selftest_sort) against the numpy reference of tests/_scatter_prim.py.

Exact class: 2^k + 1 grids, coordinates -1 + m / 2^k, small integer values and pre-fills: every term is a multiple of 2^-12 and
sum |terms| 2^12 < 2^24 per output element (asserted by the reference), so no summation order, atomic order, run reduction, LDS
or global accumulation, window placement or sort order can change a bit: torch.equal with the int64 fixed-point sums for the ray,
sorted and sorted_plain forms.  Dense class: normal values on odd grids, e = |g - g64| / sum |terms| within 2 x the same metric
of a sequential fp32 evaluation.  Workspaces are filled with 0xFF before every call; gradient tensors sit in one flat buffer with
guard gaps that must keep their fill."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import _scatter_prim as P
from _twin import CHILD, run_twin
from _util import pkg, record_margin

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = {"ray": 0, "sorted": 1, "sorted_plain": 3}
GAP = -2.0
VISITED = set()          # launch-policy branches the file has seen taken (rdrf_selftest_scatter_last)
MARGINS = []
DET = None               # tests/_det_child.py: binds every call's gradient buffer to a fixed-point shadow (deterministic library)


def _modes(desc):
    return ("ray", "sorted", "sorted_plain") if desc["rec_floats"] else ("ray",)


_DESC = {}


def _desc(kind, grid):
    key = (kind, tuple(grid))
    if key not in _DESC:
        _DESC[key] = P.describe(pkg(), kind, list(grid))
    return _DESC[key]


class Dev:
    """a case on the device: factor values, and every output as a view of one flat buffer with 64-float guard gaps"""

    def __init__(self, case, order="W"):
        L = pkg()
        self.case, self.order, d = case, order, case["desc"]
        self.d = d
        self.shapes = P.shapes(case)
        self.slices, n = {}, 64
        for k, shp in self.shapes.items():
            size = int(np.prod(shp))
            self.slices[k] = slice(n, n + size)
            n += (size + 127) // 64 * 64
        self.total = n
        self.flat = torch.zeros(self.total, device="cuda")
        self.vals = {}
        self.t = L.RdrfScatterTest()
        for set_ in range(d["nsets"]):
            for p, (W, H, Ln) in enumerate(P.plane_dims(case["grid"])):
                Cn = d["C"][p]
                pl = torch.from_numpy(self.phys(case["planes"][set_][p])).float().contiguous().cuda()
                ln = torch.from_numpy(case["lines"][set_][p]).float().contiguous().cuda()
                self.vals[(set_, p)] = (pl, ln)
                for vm, a, b in ((self.t.vm[set_], pl.data_ptr(), ln.data_ptr()),
                                 (self.t.gvm[set_], self.flat.data_ptr() + 4 * self.slices[("plane", set_, p)].start,
                                  self.flat.data_ptr() + 4 * self.slices[("line", set_, p)].start)):
                    vm.plane[p], vm.line[p], vm.C[p], vm.H[p], vm.W[p], vm.L[p] = a, b, Cn, H, W, Ln
                    vm.sH[p], vm.sW[p] = (W * Cn, Cn) if order == "W" else (Cn, H * Cn)
        self.t.set_mask, self.t.N, self.t.S, self.t.flat = case["set_mask"], case["N"], case["S"], case["flat"]
        self.coords = torch.from_numpy(np.ascontiguousarray(case["coords"])).cuda()
        self.valid = torch.from_numpy(case["valid"]).cuda()
        self.t.coords, self.t.valid = self.coords.data_ptr(), self.valid.data_ptr()
        for i in range(3):
            self.t.box_lo[i], self.t.box_inv[i] = case["box_lo"][i], case["box_inv"][i]
        ns = case["N"] * case["S"]
        if d["list"]:
            lst = np.full(ns, 0x7fffffff, dtype=np.int32)          # entries past the count must never be used as sample ids
            lst[: case["count"]] = case["list"]
            self.list = torch.from_numpy(lst).cuda()
            self.count = torch.tensor([case["count"]], dtype=torch.int32, device="cuda")
            self.t.list, self.t.count = self.list.data_ptr(), self.count.data_ptr()
        self.rows = torch.from_numpy(P.layout_rows(case)).cuda()
        self.t.rows, self.t.rows_floats = self.rows.data_ptr(), self.rows.numel()
        if d["rec_floats"]:
            self.recs = torch.from_numpy(P.layout_recs(case)).cuda()
            self.t.recs, self.t.recs_floats = self.recs.data_ptr(), self.recs.numel()
            self.ws = torch.empty(L.lib.rdrf_selftest_scatter_workspace_bytes(case["N"], case["S"]), dtype=torch.uint8, device="cuda")
            self.t.ws, self.t.ws_bytes = self.ws.data_ptr(), self.ws.numel()
            self.keys = torch.empty(3 * ns, dtype=torch.int32, device="cuda")
            self.keys_in = torch.empty(3 * ns, dtype=torch.int32, device="cuda")
            self.t.keys_out = self.keys_in.data_ptr()
            self.ordr = torch.empty(3 * ns, dtype=torch.int32, device="cuda")
            self.cnts = torch.empty(3, dtype=torch.int32, device="cuda")
            self.t.keys_sorted_out, self.t.order_out, self.t.counts_out = self.keys.data_ptr(), self.ordr.data_ptr(), self.cnts.data_ptr()
        self.t.dxw = self.flat.data_ptr() + 4 * self.slices["dxw"].start
        self.t.g_xyz = self.flat.data_ptr() + 4 * self.slices["g_xyz"].start

    def phys(self, a):
        return np.ascontiguousarray(a if self.order == "W" else np.transpose(a, (1, 0, 2)))

    def flatten(self, arrays):
        out = np.full(self.total, GAP, dtype=np.float64)
        for k, sl in self.slices.items():
            a = np.asarray(arrays[k], dtype=np.float64)
            out[sl] = (self.phys(a) if k[0] == "plane" else a).ravel()
        return out

    def call(self, mode, pre, check=True):
        L = pkg()
        self.flat.copy_(torch.from_numpy(self.flatten(pre)).float())
        if self.d["rec_floats"]:
            self.ws.fill_(0xFF)
            self.keys.fill_(-1), self.ordr.fill_(-1), self.cnts.fill_(-1), self.keys_in.fill_(-1)
        if DET is not None:
            DET.bind(self)
        rc = L.lib.rdrf_selftest_scatter(L.SCATTER_KINDS[self.d["kind"]], MODES[mode], C.byref(self.t), L.stream_of(self.flat))
        torch.cuda.synchronize()
        if DET is not None and rc == 0:
            DET.finish(self)
        if check:
            L.check(rc, f"rdrf_selftest_scatter {self.d['kind']} {mode}")
            self.last = last_record()
            visit(self.last)
        return rc

    def where(self, got, want):
        msgs = []
        covered = np.zeros(self.total, dtype=bool)
        for k, sl in self.slices.items():
            covered[sl] = True
            bad = np.nonzero(got[sl] != want[sl])[0]
            if len(bad):
                shp = self.shapes[k] if (k[0] != "plane" or self.order == "W") else (self.shapes[k][1], self.shapes[k][0], self.shapes[k][2])
                idx = tuple(int(i) for i in np.unravel_index(bad[0], shp))
                msgs.append(f"{k}: {len(bad)} of {sl.stop - sl.start} differ, first at {idx} (storage order {self.order}): "
                            f"{got[sl][bad[0]]} != {want[sl][bad[0]]}")
        gap = np.nonzero((got != want) & ~covered)[0]
        if len(gap):
            msgs.append(f"{len(gap)} guard floats were written, first flat index {gap[0]}")
        return "; ".join(msgs)

    def stage_check(self, what):
        """sorted modes: name the first stage that differs from the reference (key generation, sort, count search)"""
        keys, ks, order, counts = P.reference_keys(self.case)
        n = len(ks)
        gi = self.keys_in.cpu().numpy().view(np.uint32)[:n]
        assert np.array_equal(gi, keys), f"{what}: stage KEY GENERATION: keys differ at {np.nonzero(gi != keys)[0][:4]}"
        gk = self.keys.cpu().numpy().view(np.uint32)[:n]
        go = self.ordr.cpu().numpy().view(np.uint32)[:n]
        gc = self.cnts.cpu().tolist()
        assert np.array_equal(gk, ks), f"{what}: stage SORT: sorted keys differ at {np.nonzero(gk != ks)[0][:4]}"
        assert np.array_equal(go, order), f"{what}: stage SORT (stability): order differs at {np.nonzero(go != order)[0][:4]}"
        assert gc == counts, f"{what}: stage COUNT SEARCH: {gc} != {counts}"


def last_record():
    L = pkg()
    buf = (C.c_int * 32)()
    n = L.lib.rdrf_selftest_scatter_last(buf, 32)
    assert n >= 4 and buf[0] == n
    launches = [dict(zip(("elem", "threads", "wgs", "tiled", "tw", "steps"), buf[4 + 6 * i: 10 + 6 * i])) for i in range(buf[3])]
    return dict(form=buf[1], split=buf[2], launches=launches)


def visit(rec):
    for l in rec["launches"]:
        if rec["form"] == 0:
            VISITED.add(("ray", l["elem"], "split" if rec["split"] else "one"))
            VISITED.add(("ray threads", l["threads"]))
        else:
            VISITED.add(("sorted", {1: "tiled", 0: "refused", -2: "off", -1: "plain"}[l["tiled"]], l["elem"]))


def int_prefill(case, seed=9):
    rng = np.random.default_rng(seed)
    return {k: rng.integers(-3, 4, s).astype(np.float64) for k, s in P.shapes(case).items()}


def exact(case, what, orders=("W",), modes=None, pre=None, stage=True):
    """every mode of the kind gives the bits of the int64 reference; returns the flat results per (order, mode)"""
    d = case["desc"]
    pre = int_prefill(case) if pre is None else pre
    out = {}
    for order in orders:
        dev = Dev(case, order)
        for mode in modes or _modes(d):
            ref, _ = P.reference(case, mode, "exact", pre)
            want = dev.flatten(ref)
            dev.call(mode, pre)
            got = dev.flat.cpu().double()
            if mode != "ray" and stage:
                dev.stage_check(f"{d['kind']} {mode} {what}")
            if not torch.equal(got, torch.from_numpy(want)):
                pytest.fail(f"{d['kind']} {mode} {what}: stage SCATTER: {dev.where(got.numpy(), want)}")
            out[(order, mode)] = got
    return out


def dyadic_case(kind, grid, N, S, seed=0, coords=None, **kw):
    d = _desc(kind, grid)
    rng = np.random.default_rng(seed)
    coords = P.dyadic_coords(rng, grid, N * S) if coords is None else coords
    kw.setdefault("mag", 1)
    return P.make_case(d, grid, N, S, coords, rng, **kw)


# ---- sort ----------------------------------------------------------------------------------------------------------------------
SORT_N = [1, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 4097, 3 * 2048 + 1]
SORT_BITS = [1, 9, 10, 18, 19, 27, 28]


def _sort_call(keys, bits, count=None, n_mul=0):
    L = pkg()
    n = len(keys)
    k = torch.from_numpy(keys.view(np.int32)).cuda()
    ko = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    oo = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    tmp = torch.full((L.lib.rdrf_selftest_sort_temp_bytes(n, bits),), 0xFF, dtype=torch.uint8, device="cuda")
    cnt = None if count is None else torch.tensor([count], dtype=torch.int32, device="cuda")
    rc = L.lib.rdrf_selftest_sort(L.ptr(k), n, bits, L.ptr(cnt), n_mul, L.ptr(ko), L.ptr(oo), L.ptr(tmp), tmp.numel(), L.stream_of(k))
    torch.cuda.synchronize()
    L.check(rc, "rdrf_selftest_sort")
    return ko.cpu().numpy().view(np.uint32), oo.cpu().numpy().view(np.uint32)


def _patterns(n, bits, rng):
    top = (1 << bits) - 1
    hot = rng.integers(0, top + 1, n, dtype=np.uint64)
    hot[rng.random(n) < 0.7] = top // 3
    return {"equal": np.full(n, top, dtype=np.uint64), "two": np.where(np.arange(n) % 2, top, top // 2).astype(np.uint64),
            "ascending": np.arange(n, dtype=np.uint64) % (top + 1), "descending": (n - 1 - np.arange(n, dtype=np.uint64)) % (top + 1),
            "random": rng.integers(0, top + 1, n, dtype=np.uint64), "hot": hot}


@pytest.mark.parametrize("n", SORT_N)
def test_sort_is_stable_and_exact_at_round_tile_and_pass_edges(n):
    rng = np.random.default_rng(n)
    for bits in SORT_BITS:
        for name, k in _patterns(n, bits, rng).items():
            keys = k.astype(np.uint32)
            want_k, want_o = P.reference_sort(keys, bits)
            got_k, got_o = _sort_call(keys, bits)
            assert np.array_equal(got_k, want_k), f"n {n} bits {bits} {name}: keys differ at {np.nonzero(got_k != want_k)[0][:4]}"
            assert np.array_equal(got_o, want_o), f"n {n} bits {bits} {name}: not stable at {np.nonzero(got_o != want_o)[0][:4]}"


@pytest.mark.parametrize("count", [0, 1, 682, 683, 684, 1365, 1366, 2000])
def test_sort_with_a_device_count_leaves_the_rest_alone(count):
    """3 * count just below, at and above the 2048-entry tile edge (682, 683) and the two-tile edge; 3 * 2000 > n: the clamp"""
    n, bits = 4097, 18
    rng = np.random.default_rng(count)
    keys = rng.integers(0, 1 << bits, n, dtype=np.uint64).astype(np.uint32)
    m = min(n, 3 * count)
    want_k, want_o = P.reference_sort(keys, bits, m)
    got_k, got_o = _sort_call(keys, bits, count, 3)
    assert np.array_equal(got_k[:m], want_k) and np.array_equal(got_o[:m], want_o)
    assert (got_k[m:] == 0xffffffff).all() and (got_o[m:] == 0xffffffff).all()      # the sentinel fill of this test


# ---- keys and counts -----------------------------------------------------------------------------------------------------------
def test_keys_and_counts_at_the_edges_of_the_grid():
    grid = [9, 17, 9]
    e = 2.0 ** -20
    edge = [-1.0, -1.0 + e, -1.0 - e, 1.0, 1.0 - e, 1.0 + e, 1.6, -1.6, 2.5, -2.5, 1e30, -1e30, 0.25]
    coords = np.array([[a if ax == i else 0.25 for i in range(3)] for ax in range(3) for a in edge], dtype=np.float32)
    n = len(coords)
    valid = np.ones(n, dtype=np.uint8)
    valid[[3, 20]] = 0
    case = dyadic_case("DYN_DENSITY", grid, 1, n, coords=coords, valid=valid, sm_dead=[5, 30], flat=1, density=0.0)
    dev = Dev(case)
    dev.call("sorted_plain", int_prefill(case))
    dev.stage_check("edge coordinates")
    assert P.reference_keys(case)[3] != [n, n, n]


@pytest.mark.parametrize("count", [0, 1, 31, 32, 33])
def test_compact_list_keys_and_scatter(count):
    rng = np.random.default_rng(count)
    case = dyadic_case("DYN_APP", [9, 9, 9], 2, 33, seed=count, list_=rng.permutation(66)[:count])
    exact(case, f"count {count}")


# ---- scatter: shapes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 31, 32, 33, 65])
@pytest.mark.parametrize("kind", P.KINDS)
def test_scatter_shapes_are_exact_in_every_mode(kind, S):
    """one tile (three of a workgroup's four waves find none) and nine rays; half of the samples dead; an unsorted list with
    counts around 32 and around one workgroup's share (4 waves x 32); ray and flat tiles; the dxw / g_xyz pre-fill is non-zero.
    Tiles per wave: 0 and 1 here.  A second iteration of the static-stride tile loop needs more tiles than the capped grid holds
    (768 workgroups x 4 waves): test_more_tiles_than_the_capped_grid_holds runs it for the dynamic and the static density kernels;
    for the two appearance kernels it would take 3073 x 544 saved rows (214 MB) and a 216-feature reference of 98 k samples, which
    is no few-second test: their tile loop is the same source line of the one k_scatter template and stays uncovered."""
    grid = [9, 17, 9]
    for N in (1, 9):
        d = _desc(kind, grid)
        rng = np.random.default_rng(100 * S + N)
        ns = N * S
        kw = {}
        if d["list"]:
            kw["list_"] = rng.permutation(ns)[: max(1, min(ns, {1: 31, 9: 129}[N] + S % 3))]
        else:
            kw["valid"] = rng.random(ns) < 0.5
        if kind == "DYN_DENSITY":
            for flat, mask in ((0, 3), (1, 3), (1, 1), (1, 2), (0, 2)):
                case = dyadic_case(kind, grid, N, S, seed=S, flat=flat, set_mask=mask, **kw)
                exact(case, f"N {N} S {S} flat {flat} mask {mask}", modes=_modes(d) if flat else ("ray",))
        else:
            exact(dyadic_case(kind, grid, N, S, seed=S, **kw), f"N {N} S {S}")


def test_more_tiles_than_the_capped_grid_holds():
    """dynamic density: 3 x 256 workgroups x 4 waves = 3072 tiles resident; 3201 flat tiles make the static stride wrap"""
    grid = [17, 17, 17]
    N, S = 1067, 96
    assert (N * S + 31) // 32 > 3072
    case = dyadic_case("DYN_DENSITY", grid, N, S, flat=1, density=0.01)
    exact(case, "wrap", modes=("ray", "sorted"))
    dev_wgs = [l["wgs"] for l in last_record()["launches"]]
    assert max(dev_wgs) <= 768
    N = 3100                                                  # static density: one ray tile per ray, 3100 > 3072
    case = dyadic_case("STATIC_DENSITY", grid, N, 32, density=0.05)
    exact(case, "wrap, static density")
    assert last_record()["launches"][0]["wgs"] == 768


# ---- scatter: designed trajectories --------------------------------------------------------------------------------------------
STEPS = {"stay": (0, 0), "+x": (1, 0), "-x": (-1, 0), "+y": (0, 1), "-y": (0, -1), "++": (1, 1), "+-": (1, -1), "-+": (-1, 1),
         "--": (-1, -1), "jump": (5, 3)}
LANES = (0, 1, 14, 15, 16, 17, 30, 31)


def _trajectories(grid):
    """32-sample tiles of cell walks: every ordered pair of steps placed at the lane positions that cross the 16-lane row, the
    half-wave edge and the tile ends (three-run chains A, B, C and A, B, A among them); runs of every length 1 .. 32 walking +x,
    -x, +y, -y; the same with a dead sample at the head, in the middle and at the tail of every run.  Returns cells [tiles][32][2]
    and valid [tiles][32]."""
    tiles, valid = [], []
    t = 0
    for a in STEPS.values():
        for b in STEPS.values():
            for pos in LANES:
                base = np.array([3 + t % 9, 3 + (t // 9) % 9])
                cells = np.tile(base, (32, 1))
                cells[pos:] += a
                if pos + 1 < 32:
                    cells[pos + 1:] += b
                tiles.append(cells)
                valid.append(np.ones(32, dtype=np.uint8))
                t += 1
    for r in range(1, 33):
        for d_ in ((1, 0), (-1, 0), (0, 1), (0, -1)):
            run = (np.arange(32) // r) % 13                        # (a walk longer than the grid starts again: one more jump)
            start = np.array([8, 8]) - 6 * np.array(d_)
            cells = start[None, :] + run[:, None] * np.array(d_)[None, :]
            for kill in (None, 0, r // 2, r - 1):
                v = np.ones(32, dtype=np.uint8)
                if kill is not None:
                    v[(np.arange(32) % r) == kill] = 0
                tiles.append(cells)
                valid.append(v)
    return np.stack(tiles), np.stack(valid)


def _trajectory_coords(grid, cells, rng):
    """x, y follow the walk, z follows y (XZ sees the walk itself, YZ its diagonal); half-cell offsets inside a cell"""
    n = cells.shape[0] * 32
    cx, cy = cells[..., 0].reshape(n), cells[..., 1].reshape(n)
    out = np.zeros((n, 3), dtype=np.float32)
    for a, cell in enumerate((cx, cy, cy)):
        k = int(np.log2(grid[a] - 1))
        out[:, a] = -1.0 + (2 * cell + rng.integers(0, 2, n)) / float(1 << k)
    return out


@pytest.mark.parametrize("part", [0, 1])
@pytest.mark.parametrize("order", ["W", "H"])
@pytest.mark.parametrize("kind", P.KINDS)
def test_designed_trajectories_are_exact(kind, order, part):
    """no factor value and no d(feature) of a designed sample is zero (values +-1), so a tap dropped or doubled at any one placement
    changes a sum; the headroom is kept by running 82 tiles per call (part: the first / second half of the tiles)"""
    grid = [17, 17, 17]
    d = _desc(kind, grid)
    cells, valid = _trajectories(grid)
    T = cells.shape[0]
    rng = np.random.default_rng(7)
    coords = _trajectory_coords(grid, cells, rng)
    flats = (0, 1) if kind == "DYN_DENSITY" else (0,)
    CH = 82                                                        # tiles per call: keeps sum |terms| inside the headroom
    half = (T // 2 + CH - 1) // CH * CH
    for flat in flats:
        for c0 in range(0, half, CH) if part == 0 else range(half, T, CH):
            sl = slice(c0 * 32, min(T, c0 + CH) * 32)
            n = (sl.stop - sl.start) // 32
            kw = dict(list_=np.nonzero(valid.reshape(-1)[sl])[0]) if d["list"] else dict(valid=valid.reshape(-1)[sl])
            case = dyadic_case(kind, grid, n, 32, seed=3, coords=coords[sl], flat=flat, nonzero=True, **kw)
            only_ray = d["rec_floats"] == 0 or (kind == "DYN_DENSITY" and not flat)
            exact(case, f"trajectories, tiles {c0}.., flat {flat}", orders=(order,), modes=("ray",) if only_ray else None, stage=False)


# ---- launch policy -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gz,elem,split", [(9, 8, 0), (513, 8, 1), (1025, 4, 1), (2049, 0, 0)])
def test_ray_launch_policy_branches(gz, elem, split):
    grid = [9, 9, gz]
    case = dyadic_case("DYN_DENSITY", grid, 3, 33, seed=gz, flat=1, density=0.5)
    dev = Dev(case)
    pre = int_prefill(case)
    ref, _ = P.reference(case, "ray", "exact", pre)
    dev.call("ray", pre)
    rec = dev.last
    assert rec["form"] == 0 and rec["split"] == split and len(rec["launches"]) == 1 + split, rec
    assert all(l["elem"] == elem and l["tiled"] == -1 for l in rec["launches"]), rec
    want = dev.flatten(ref)
    got = dev.flat.cpu().double()
    assert torch.equal(got, torch.from_numpy(want)), dev.where(got.numpy(), want)


def test_sorted_launch_policy_takes_and_refuses_the_windows():
    """grid [9, 9, 257]: the z lines of two factor sets (2 x 257 x 20 doubles = 80.3 KiB) and the 16-component windows of the XY pass do not
    leave room for two workgroups per CU: that pass falls back to the plain sorted kernel, the XZ / YZ passes take their windows"""
    case = dyadic_case("DYN_DENSITY", [9, 9, 257], 4, 40, flat=1)
    out = exact(case, "refusal", modes=("sorted",))
    rec = last_record()
    assert rec["form"] == 1 and [l["tiled"] for l in rec["launches"]] == [0, 1, 1], rec
    assert rec["launches"][1]["tw"] == 32 and rec["launches"][1]["steps"] == 16 and rec["launches"][0]["elem"] == 8
    exact(case, "plain", modes=("sorted_plain",))
    assert [l["tiled"] for l in last_record()["launches"]] == [-2, -2, -2]
    exact(dict(case, set_mask=1), "one set", modes=("sorted",))
    assert [l["tiled"] for l in last_record()["launches"]] == [1, 1, 1]     # one set's lines leave room
    del out


@pytest.mark.parametrize("gz,elem", [(513, 4), (1025, 0)])
def test_sorted_passes_with_lines_too_long_for_doubles_or_for_the_lds(gz, elem):
    """the XY pass accumulates the z line of both sets: 2 x 513 x 20 elements fit the LDS as floats only, 2 x 1025 x 20 not at all
    (global atomics); one set's 513-entry line fits as doubles"""
    case = dyadic_case("DYN_DENSITY", [9, 9, gz], 3, 33, seed=gz, flat=1, density=0.5)
    for mode, state in (("sorted", 0), ("sorted_plain", -2)):
        exact(case, f"gz {gz}", modes=(mode,))
        rec = last_record()["launches"]
        assert [l["tiled"] for l in rec] == [state, 1 if state == 0 else -2, 1 if state == 0 else -2], rec
        assert rec[0]["elem"] == elem and rec[0]["threads"] == 512, rec
    exact(dict(case, set_mask=2), f"gz {gz}, one set", modes=("sorted_plain",))
    assert last_record()["launches"][0]["elem"] == (8 if gz == 513 else 4)


def test_ray_launch_with_two_workgroups_per_cu():
    """appearance lines on [9, 9, 129]: 8 x (129 x 52 + 2 x 9 x 16) = 56 KB of accumulators, between the 53 KB and 80 KB steps of
    launch_scatter_k (two 256-thread workgroups per CU).  It differs from the three-per-CU branch only in the grid cap (512 / 768
    workgroups), which no few-second case reaches; the one-per-CU branch (512 threads) is the split launches above."""
    for kind in ("STATIC_APP", "DYN_APP"):
        case = dyadic_case(kind, [9, 9, 129], 2, 40, list_=np.random.default_rng(1).permutation(80)[:50])
        exact(case, "two per CU", modes=("ray",))
        rec = last_record()
        assert rec["launches"][0]["elem"] == 8 and rec["launches"][0]["threads"] == 256 and not rec["split"], rec


# ---- tiled windows -------------------------------------------------------------------------------------------------------------
def _cloud(grid, n, rng, lo, hi):
    """dyadic coordinates whose x, y cells lie in [lo, hi)"""
    out = np.zeros((n, 3), dtype=np.float32)
    for a, g in enumerate(grid):
        k = int(np.log2(g - 1))
        cell = rng.integers(lo, min(hi, g - 1), n) if a < 2 else rng.integers(0, g - 1, n)
        out[:, a] = -1.0 + (2 * cell + rng.integers(0, 2, n)) / float(1 << k)
    return out


@pytest.mark.parametrize("name", ["dense", "sparse", "narrow", "row_ends", "clamped", "slice-1", "slice", "slice+1", "slice2-1", "slice2+1"])
def test_tiled_windows_equal_plain_sorted_ray_and_reference(name):
    rng = np.random.default_rng(len(name))
    grid, n, kw = [65, 65, 9], 1000, {}
    if name == "dense":
        coords = _cloud(grid, 1920, rng, 20, 28)                     # 30 entries per level-0 cell
        n = 1920
    elif name == "sparse":
        coords = _cloud(grid, 600, rng, 0, 64)                       # most of the 4096 cells empty, slices span several rows
        n = 600
    elif name == "narrow":
        grid = [17, 17, 9]                                           # W < tw: the whole plane in one window
        coords = _cloud(grid, n, rng, 0, 16)
    elif name == "row_ends":
        coords = _cloud(grid, n, rng, 61, 64)                        # slices begin in the last cells of a key row
        coords[:, 1] = _cloud(grid, n, rng, 0, 64)[:, 1]
    elif name == "clamped":
        coords = _cloud(grid, n, rng, 0, 64)
        coords[::5, 0] = rng.choice([1.25, -1.25, 1.5, -1.0625], n)[::5]      # level-0 taps out of range, coarser ones in
        coords[::7, 1] = 1.125
    else:
        n = {"slice-1": 255, "slice": 256, "slice+1": 257, "slice2-1": 511, "slice2+1": 513}[name]
        coords = _cloud(grid, n, rng, 10, 40)
    case = dyadic_case("DYN_DENSITY", grid, 1, n, seed=1, coords=coords, flat=1, density=0.3, **kw)
    out = exact(case, name)
    rec_ok = out[("W", "sorted")]
    assert torch.equal(rec_ok, out[("W", "sorted_plain")]) and torch.equal(rec_ok, out[("W", "ray")])
    Dev(case).call("sorted", int_prefill(case))
    assert [l["tiled"] for l in last_record()["launches"]] == [1, 1, 1]


# ---- dense class ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [[17, 19, 11], [23, 13, 29]], ids=["17x19x11", "23x13x29"])
@pytest.mark.parametrize("kind", P.KINDS)
def test_dense_values_stay_within_twice_the_sequential_fp32_error(kind, grid):
    d = _desc(kind, grid)
    case = P.dense_case(d, grid)
    pre = {k: np.zeros(s) for k, s in P.shapes(case).items()}
    dev = Dev(case)
    for mode in _modes(d):
        g64, mag = P.reference(case, mode, "f64", pre)
        s32, _ = P.reference(case, mode, "seq32", pre)
        dev.call(mode, pre)
        got = dev.flat.cpu().double().numpy()
        worst = 0.0
        for k, sl in dev.slices.items():
            m = mag[k].ravel()
            if not (m > 0).any():
                continue
            ref = (dev.phys(g64[k]) if k[0] == "plane" else g64[k]).ravel()
            seq = (dev.phys(s32[k]) if k[0] == "plane" else s32[k]).ravel()
            mm = (dev.phys(mag[k]) if k[0] == "plane" else mag[k]).ravel()
            nz = mm > 0
            e = (np.abs(got[sl] - ref)[nz] / mm[nz]).max()
            e_seq = (np.abs(seq - ref)[nz] / mm[nz]).max()
            ratio = e / e_seq
            print(f"{kind} {grid} {mode} {k}: e {e:.3e} e_seq32 {e_seq:.3e} ratio {ratio:.3f}")
            MARGINS.append(f"{kind:15s} {'x'.join(map(str, grid)):9s} {mode:12s} {str(k):18s} e {e:.3e}  e_seq32 {e_seq:.3e}  ratio {ratio:.3f}")
            worst = max(worst, ratio)
            assert (got[sl][~nz] == 0).all()
        record_margin(f"scatter_prim.{kind}.{'x'.join(map(str, grid))}.{mode}", worst / 2.0)
        assert worst <= 2.0, (kind, grid, mode, worst)
    if os.environ.get("RDRF_SCATTER_MARGINS"):       # the table of profiles/scatter_primitives_margins.txt
        with open(os.environ["RDRF_SCATTER_MARGINS"], "a") as f:
            f.write("\n".join(MARGINS) + "\n")
        del MARGINS[:]


# ---- error paths ---------------------------------------------------------------------------------------------------------------
def test_error_paths():
    L = pkg()
    case = dyadic_case("DYN_DENSITY", [9, 9, 9], 2, 33, flat=1)
    dev = Dev(case)
    pre = int_prefill(case)
    st = L.stream_of(dev.flat)
    call = lambda kind, mode: L.lib.rdrf_selftest_scatter(kind, mode, C.byref(dev.t), st)
    assert call(7, 0) == -1 and b"unknown kind" in L.lib.rdrf_last_error()
    assert call(1, 2) == -1 and call(1, 9) == -1                         # auto is no mode of the self-test
    assert call(0, 1) == -2 and call(2, 3) == -2                         # the static kinds have no sorted form
    dev.t.flat = 0
    assert call(1, 1) == -2                                              # the sorted density passes run on flat tiles
    dev.t.flat = 1
    dev.t.ws_bytes -= 1
    assert call(1, 1) == -3 and b"workspace" in L.lib.rdrf_last_error()
    dev.t.ws_bytes += 1
    dev.t.recs += 4
    assert call(1, 1) == -1 and b"aligned" in L.lib.rdrf_last_error()
    dev.t.recs -= 4
    dev.t.rows_floats -= 1
    assert call(1, 0) == -3
    dev.t.rows_floats += 1
    dev.t.set_mask = 0
    assert call(1, 0) == -1
    dev.t.set_mask = 3
    dev.t.vm[1].W[0] += 1
    assert call(1, 0) == -1
    dev.t.vm[1].W[0] -= 1
    torch.cuda.synchronize()
    assert dev.call("sorted", pre) == 0                                  # the description is intact again
    app = Dev(dyadic_case("DYN_APP", [9, 9, 9], 1, 40, list_=np.arange(8)))
    app.list[3] = 40
    assert L.lib.rdrf_selftest_scatter(3, 0, C.byref(app.t), L.stream_of(app.flat)) == -1 and b"outside the batch" in L.lib.rdrf_last_error()
    app.count[0] = 41
    assert L.lib.rdrf_selftest_scatter(3, 0, C.byref(app.t), L.stream_of(app.flat)) == -1
    k = torch.zeros(8, dtype=torch.int32, device="cuda")
    assert L.lib.rdrf_selftest_sort(L.ptr(k), 8, 0, None, 0, L.ptr(k), L.ptr(k), None, 0, st) == -1
    assert L.lib.rdrf_selftest_sort(L.ptr(k), 8, 9, None, 0, L.ptr(k), L.ptr(k), L.ptr(dev.ws), 16, st) == -3
    assert L.lib.rdrf_selftest_sort(None, 0, 9, None, 0, None, None, None, 0, st) == 0


# ---- deterministic library -----------------------------------------------------------------------------------------------------
def det_cases():
    """the exact cases the deterministic library repeats (tests/_det_child.py scatter): every kind and mode at one and nine rays,
    both storage orders; a compact list; a window case; the grids of the launch-policy branches, where that build must take
    neither LDS accumulators, nor the per-set split, nor the windows; one chunk of the designed walks per kind"""
    n = 0
    for kind in P.KINDS:
        d = _desc(kind, [9, 17, 9])
        for N in (1, 9):
            rng = np.random.default_rng(N)
            kw = dict(list_=rng.permutation(N * 33)[: min(N * 33, 130)]) if d["list"] else dict(valid=rng.random(N * 33) < 0.5)
            exact(dyadic_case(kind, [9, 17, 9], N, 33, seed=N, flat=1 if d["flat"] else 0, **kw), f"det N {N}", orders=("W", "H"))
            n += 1
        cells, valid = _trajectories([17, 17, 17])
        sl = slice(0, 82 * 32)
        coords = _trajectory_coords([17, 17, 17], cells, np.random.default_rng(7))[sl]
        kw = dict(list_=np.nonzero(valid.reshape(-1)[sl])[0]) if d["list"] else dict(valid=valid.reshape(-1)[sl])
        exact(dyadic_case(kind, [17, 17, 17], 82, 32, seed=3, coords=coords, flat=1 if d["flat"] else 0, nonzero=True, **kw), "det walks",
              stage=False)
        n += 1
    rng = np.random.default_rng(5)
    exact(dyadic_case("DYN_DENSITY", [65, 65, 9], 1, 1920, seed=1, coords=_cloud([65, 65, 9], 1920, rng, 20, 28), flat=1, density=0.3), "det dense cloud")
    n += 1
    for gz in (9, 257, 513, 1025):
        exact(dyadic_case("DYN_DENSITY", [9, 9, gz], 3, 33, seed=gz, flat=1, density=0.5), f"det gz {gz}", modes=("ray",))
        rec = last_record()
        assert rec["split"] == 0 and [l["elem"] for l in rec["launches"]] == [0], rec
        exact(dyadic_case("DYN_DENSITY", [9, 9, gz], 3, 33, seed=gz, flat=1, density=0.5), f"det gz {gz}", modes=("sorted",))
        rec = last_record()
        assert [(l["elem"], l["tiled"]) for l in rec["launches"]] == [(0, -2)] * 3, rec
        n += 1
    return n


def test_same_bits_in_the_deterministic_library(tmp_path):
    """librodynrf_det.so in a child process (the library is chosen at import), the flat gradient buffer of every call bound to a
    fixed-point shadow as the fields bind theirs: after the fold, the int64 sums again, bit for bit; before it, no plane or line
    element has moved (an addition that missed the shadow)"""
    assert run_twin(tmp_path, [CHILD, "scatter"], det=True) == 3 * len(P.KINDS) + 1 + 4


# ---- last: every branch of the launch policy was really taken ------------------------------------------------------------------
def test_the_file_visited_every_launch_policy_branch():
    want = {("ray", 8, "one"), ("ray", 8, "split"), ("ray", 4, "split"), ("ray", 0, "one"), ("ray threads", 256), ("ray threads", 512),
            ("sorted", "tiled", 8), ("sorted", "refused", 8), ("sorted", "refused", 4), ("sorted", "refused", 0),
            ("sorted", "off", 8), ("sorted", "off", 4), ("sorted", "off", 0), ("sorted", "plain", 8)}
    assert want <= VISITED, f"not taken: {sorted(want - VISITED, key=str)}"
