"""k_dw3 and dw_launch on their own (rdrf_selftest_dw: the product's dW job lists on rows the test supplies) against a numpy
int64 / float64 reference built from rdrf_selftest_dw_describe alone (tests/_dw_prim.py).

(a) integer rows in [-4, 4], integer pre-fill: every partial sum is an integer below 2^24 in any order, so atomics, MFMA order
    and the launch cut cannot change a bit -- torch.equal with the int64 sums for every parameter of every plan, at every tile
    count that gives a workgroup 0 / 1 / 2 / 3 / 4 tiles, both buffer parities at loop exit and a grid below 256, and at
    device counts around the tile and grid edges.  Bias gradients, columns past in_dim and rows past out_dim are part of it.
(b) one (job, out block, input block) product at a time at two tiles: only that dz block and that input block are non-zero
    (all-ones significands of at most 11 bits, four non-zero samples per row: exact); a wrong block remap, segment base or
    bridged hole names the product it breaks.
(c) dense normal rows: e = max |dW - dW64| / sum |dz| |in| within 2 x e_seq32, the same metric of a sequential fp32
    accumulation of the same terms in sample order (numpy; a sample of out rows per job, so the bound is, if anything, low).
(d) the row contract of rdrf_dw.hip from the kernel's side: 3e38 in the activation slots past `count` changes no bit.
(e) error paths; the deterministic library gives the bits of (a)."""
import ctypes as C

import numpy as np
import pytest
import torch

import _dw_prim as P
from _twin import CHILD, run_twin
from _util import pkg, profile_line, record_margin

pytestmark = pytest.mark.gpu

ALL_PLANS = P.PLANS + [("DENSITY", f) for f in P.DENSITY_FLAGS if f != 3]
DENSITY_PLANS = [("DENSITY", f) for f in P.DENSITY_FLAGS]


def _ids(plans):
    return [f"{p}-{f}" for p, f in plans]


class Plan:
    """a plan's description, and its gradient tensors as views of one flat cuda buffer behind the struct the product passes"""

    def __init__(self, plan, flags):
        L = pkg()
        self.plan, self.flags = plan, flags
        self.desc = P.describe(L, plan, flags)
        self.cls = L.RdrfDynamicParams if self.desc["dynamic"] else L.RdrfStaticParams
        self.names = P.field_names(self.cls)
        self.shapes = P.param_shapes(self.desc)
        self.slices, n = {}, 64
        for off, shp in sorted(self.shapes.items()):
            size = int(np.prod(shp))
            self.slices[off] = slice(n, n + size)
            n += (size + 127) // 64 * 64          # at least 64 floats of nobody's between two parameters
        self.total = n
        self.flat = torch.zeros(self.total, device="cuda")
        self.struct = self.cls()
        raw = (C.c_uint64 * (C.sizeof(self.cls) // 8)).from_buffer(self.struct)
        for off, sl in self.slices.items():
            raw[off // 8] = self.flat.data_ptr() + 4 * sl.start
        self.uses_count = [bool(u) for _, _, u in self.desc["regions"]]

    def flatten(self, arrays, gap=0.0):
        out = np.full(self.total, gap, dtype=np.float64)
        for off, sl in self.slices.items():
            out[sl] = np.asarray(arrays[off], dtype=np.float64).ravel()
        return out

    def rows(self, parts):
        """per-region [ntiles][stride][32] cuda arrays -> one flat fp32 array, region g + 1 behind region g"""
        return torch.cat([p.reshape(-1).float() for p in parts]).contiguous()

    def call(self, A, B, ntiles, count=None, pre=None, check=True):
        """A, B: flat cuda rows; pre: flat float64 numpy pre-fill (None: keep).  Returns (rc, flat gradients)"""
        L = pkg()
        if pre is not None:
            self.flat.copy_(torch.from_numpy(pre).float())
        cnt = None if count is None else torch.tensor([count], dtype=torch.int32, device="cuda")
        rc = L.lib.rdrf_selftest_dw(L.DW_PLANS[self.plan], self.flags, L.ptr(A), C.c_size_t(A.numel()), L.ptr(B),
                                    C.c_size_t(B.numel()), ntiles, L.ptr(cnt), C.byref(self.struct), L.stream_of(self.flat))
        torch.cuda.synchronize()
        if check:
            L.check(rc, f"rdrf_selftest_dw {self.plan} {self.flags}")
        return rc, self.flat

    def where(self, got, want):
        """first differences between two flat arrays, by parameter name and index"""
        got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
        msgs = []
        covered = np.zeros(self.total, dtype=bool)
        for off, sl in self.slices.items():
            covered[sl] = True
            bad = np.nonzero(got[sl] != want[sl])[0]
            if len(bad):
                idx = np.unravel_index(bad[0], self.shapes[off])
                msgs.append(f"{self.names[off]}{self.shapes[off]}: {len(bad)} entries differ, first at {tuple(int(i) for i in idx)}: "
                            f"{got[sl][bad[0]]} != {want[sl][bad[0]]}")
        gap = np.nonzero((got != want) & ~covered)[0]
        if len(gap):
            msgs.append(f"{len(gap)} floats between the parameters were written, first flat index {gap[0]}")
        return "; ".join(msgs)


_PLANS = {}


def _plan(plan, flags):
    if (plan, flags) not in _PLANS:
        _PLANS[(plan, flags)] = Plan(plan, flags)
    return _PLANS[(plan, flags)]


def _int_case(pl, ntiles, count=None, hostile=None):
    """integer rows of (a): per region numpy int8 arrays.  With a count, the regions that take it hold ceil(count / 32) tiles
    that count, zero dz past `count` in the last of them (activations stay +-4, or `hostile`), and one more tile of numbers
    that nobody may read."""
    A, B, tiles = [], [], []
    for g, (sa, sb, uses) in enumerate(pl.desc["regions"]):
        a = P.int_rows(0, g, sa, ntiles).copy()
        b = P.int_rows(1, g, sb, ntiles).astype(np.float32 if hostile is not None else np.int8)
        t = ntiles
        if uses and count is not None:
            t = (count + 31) // 32
            if count % 32:
                a[t - 1, :, count % 32:] = 0
                if hostile is not None:
                    b[t - 1, :, count % 32:] = hostile
        A.append(a)
        B.append(b)
        tiles.append(t)
    return A, B, tiles


def _exact(pl, ntiles, count=None, what=""):
    A, B, tiles = _int_case(pl, ntiles, count)
    assert P.partial_sum_bound(ntiles) < 2 ** 24
    pre = P.int_prefill(pl.shapes)
    want = pl.flatten(P.reference(pl.desc, A, B, tiles, pre), gap=-2.0)
    assert np.abs(want).max() < 2 ** 24 and (want == np.rint(want)).all()
    Ag, Bg = pl.rows([torch.from_numpy(a).cuda() for a in A]), pl.rows([torch.from_numpy(b).cuda() for b in B])
    _, got = pl.call(Ag, Bg, ntiles, count, pre=pl.flatten(pre, gap=-2.0))
    if not torch.equal(got.cpu().double(), torch.from_numpy(want)):
        pytest.fail(f"{pl.plan}-{pl.flags} {what}: {pl.where(got.cpu().numpy(), want)}")
    return got.clone()


# ---- (a) exact integers ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan,flags", P.PLANS, ids=P.PLAN_IDS)
def test_exact_integer_sums_host_tile_counts(plan, flags):
    pl = _plan(plan, flags)
    for ntiles in P.HOST_TILES:
        _exact(pl, ntiles, what=f"ntiles = {ntiles}")


@pytest.mark.parametrize("plan,flags", P.COUNT_PLANS, ids=_ids(P.COUNT_PLANS))
def test_exact_integer_sums_device_counts(plan, flags):
    pl = _plan(plan, flags)
    assert any(pl.uses_count)
    for count in P.COUNTS:
        _exact(pl, (count + 31) // 32 + 1, count, what=f"count = {count}")


@pytest.mark.parametrize("plan,flags", DENSITY_PLANS, ids=_ids(DENSITY_PLANS))
def test_exact_integer_sums_density_phase_flags(plan, flags):
    pl = _plan(plan, flags)
    for ntiles in (3, 257):
        _exact(pl, ntiles, what=f"ntiles = {ntiles}")


# ---- (b) one product at a time --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan,flags", ALL_PLANS, ids=_ids(ALL_PLANS))
def test_one_product_at_a_time(plan, flags):
    pl = _plan(plan, flags)
    desc, T = pl.desc, 2
    pre = P.int_prefill(pl.shapes, seed=9)
    pre_flat = pl.flatten(pre, gap=-2.0)
    regs = desc["regions"]
    Ag = [torch.zeros(T, sa, 32, device="cuda") for sa, _, _ in regs]
    Bg = [torch.zeros(T, sb, 32, device="cuda") for _, sb, _ in regs]
    An = [np.zeros((T, sa, 32), dtype=np.float32) for sa, _, _ in regs]
    Bn = [np.zeros((T, sb, 32), dtype=np.float32) for _, sb, _ in regs]
    failures = []
    triples = P.job_products(desc)
    for n, (ji, bo, k) in enumerate(triples):
        j = desc["jobs"][ji]
        g, ar, br = j["region"], j["A_row0"] + 32 * bo, j["blocks"][k][0]
        rng = np.random.default_rng([23, n])
        a = np.zeros((T, 32, 32), dtype=np.float32)
        for t in range(T):       # four non-zero samples per dz row: one in each half stage of each tile
            for half in range(2):
                s = 16 * half + int(rng.integers(0, 16))
                a[t, :, s] = P.ones_significand(rng, (32,))
        b = P.ones_significand(rng, (T, 32, 32))
        An[g][:, ar:ar + 32], Bn[g][:, br:br + 32] = a, b
        Ag[g][:, ar:ar + 32], Bg[g][:, br:br + 32] = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
        want = pl.flatten(P.reference(desc, An, Bn, [T] * len(regs), pre), gap=-2.0)
        assert np.abs(want).max() < 2 ** 24
        assert (want != pre_flat).any(), "the product owns nothing"
        _, got = pl.call(pl.rows(Ag), pl.rows(Bg), T, pre=pre_flat)
        got = got.cpu().numpy()
        if not np.array_equal(got.astype(np.float64), want):
            failures.append(f"job {ji} ({pl.names[j['w_off']]}) out block {bo} input block {k} (dz rows {ar}.., input rows {br}.., "
                            f"region {g}): {pl.where(got, want)}")
        An[g][:, ar:ar + 32], Bn[g][:, br:br + 32] = 0, 0
        Ag[g][:, ar:ar + 32], Bg[g][:, br:br + 32] = 0, 0
    assert not failures, f"{len(failures)} of {len(triples)} products wrong:\n" + "\n".join(failures[:12])


# ---- (c) accuracy on real numbers -----------------------------------------------------------------------------------------
def _e_seq32(desc, A, B, ntiles, rows_per_job=4):
    """the metric of a sequential fp32 accumulation in sample order, over rows_per_job out rows of every job (all columns,
    and the bias): max |sum32 - sum64| / sum |dz| |in|"""
    worst = 0.0
    for g in range(len(desc["regions"])):
        jobs = [j for j in desc["jobs"] if j["region"] == g]
        rows = []
        for n, j in enumerate(jobs):
            pick = np.random.default_rng([31, g, n]).choice(j["out_dim"], size=min(rows_per_job, j["out_dim"]), replace=False)
            rows.append(j["A_row0"] + j["out_row0"] + np.sort(pick))
        allrows = np.concatenate(rows)
        N = ntiles * 32
        a = np.ascontiguousarray(A[g][:, allrows].transpose(0, 2, 1).reshape(N, len(allrows)))      # [sample][row]
        b = np.ascontiguousarray(B[g].transpose(0, 2, 1).reshape(N, B[g].shape[1]))                 # [sample][input row]
        acc = np.zeros((a.shape[1], b.shape[1]), dtype=np.float32)
        bias = np.zeros(a.shape[1], dtype=np.float32)
        tmp = np.empty_like(acc)
        for s in range(N):
            np.multiply(a[s][:, None], b[s][None, :], out=tmp)
            acc += tmp
            bias += a[s]
        a64, b64 = a.astype(np.float64), b.astype(np.float64)
        ref, mag = a64.T @ b64, np.abs(a64).T @ np.abs(b64)
        rel = np.abs(acc - ref) / mag
        relb = np.abs(bias - a64.sum(axis=0)) / np.abs(a64).sum(axis=0)
        o = 0
        for j, r in zip(jobs, rows):
            for row0, cols in j["blocks"]:
                e = np.nonzero(cols >= 0)[0]
                worst = max(worst, float(rel[o:o + len(r)][:, row0 + e].max()))
            if j["b_off"] >= 0:
                worst = max(worst, float(relb[o:o + len(r)].max()))
            o += len(r)
    return worst


@pytest.mark.parametrize("ntiles", [257, 769])
@pytest.mark.parametrize("plan,flags", P.PLANS, ids=P.PLAN_IDS)
def test_dense_accuracy_against_float64(plan, flags, ntiles):
    pl = _plan(plan, flags)
    desc = pl.desc
    rng = np.random.default_rng([41, P.PLANS.index((plan, flags)), ntiles])
    A = [rng.standard_normal((ntiles, sa, 32), dtype=np.float32) for sa, _, _ in desc["regions"]]
    B = [rng.standard_normal((ntiles, sb, 32), dtype=np.float32) for _, sb, _ in desc["regions"]]
    tiles = [ntiles] * len(A)
    zero = {off: np.zeros(s) for off, s in pl.shapes.items()}
    ref = pl.flatten(P.reference(desc, A, B, tiles, zero))
    mag = pl.flatten(P.reference(desc, A, B, tiles, zero, absolute=True))
    e32 = _e_seq32(desc, A, B, ntiles)
    bound = 2.0 * e32
    _, got = pl.call(pl.rows([torch.from_numpy(a).cuda() for a in A]), pl.rows([torch.from_numpy(b).cuda() for b in B]), ntiles,
                     pre=np.zeros(pl.total))
    got = got.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    assert (got[mag == 0] == 0).all(), "an entry no product owns was written"
    own = mag > 0
    rel = np.abs(got[own] - ref[own]) / mag[own]
    e = float(rel.max())
    print(f"{plan}-{flags} ntiles = {ntiles}: e = {e:.3e}   e_seq32 = {e32:.3e}   e / e_seq32 = {e / e32:.3f}")
    profile_line("RDRF_DW_PRIM_TABLE", f"{plan:12s} {flags:2d} {ntiles:4d} {e:.3e} {e32:.3e} {e / e32:.3f}")
    record_margin(f"dW {plan}-{flags} ntiles {ntiles} e / (2 e_seq32)", e / bound)
    assert e <= bound, (f"{plan}-{flags} ntiles = {ntiles}: e = {e:.3e} > 2 x e_seq32 = {bound:.3e} (e_seq32 is the largest error of "
                        "4 sampled out rows per job, e of all rows: if this misses narrowly, compare on all rows before blaming the kernel)")


# ---- (d) the row contract, from the kernel's side -------------------------------------------------------------------------
@pytest.mark.parametrize("count", [17, 32 * 256 + 1])
@pytest.mark.parametrize("plan,flags", P.COUNT_PLANS, ids=_ids(P.COUNT_PLANS))
def test_finite_activations_behind_zero_dz_change_no_bit(plan, flags, count):
    pl = _plan(plan, flags)
    ntiles = (count + 31) // 32 + 1
    pre = pl.flatten(P.int_prefill(pl.shapes), gap=-2.0)
    out = []
    for hostile in (0.0, 3e38):
        A, B, tiles = _int_case(pl, ntiles, count, hostile=hostile)
        assert count % 32 and max(float(np.abs(b).max()) for b in B) == max(float(np.float32(hostile)), P.MAXV)
        _, got = pl.call(pl.rows([torch.from_numpy(a).cuda() for a in A]), pl.rows([torch.from_numpy(b).cuda() for b in B]),
                         ntiles, count, pre=pre)
        out.append(got.clone())
    assert bool(torch.isfinite(out[1]).all()), pl.where(out[1].cpu().numpy(), out[0].cpu().numpy())
    assert torch.equal(out[0].view(torch.int32), out[1].view(torch.int32)), pl.where(out[1].cpu().numpy(), out[0].cpu().numpy())
    A, B, tiles = _int_case(pl, ntiles, count, hostile=0.0)
    want = pl.flatten(P.reference(pl.desc, A, B, tiles, P.int_prefill(pl.shapes)), gap=-2.0)
    assert np.array_equal(out[1].cpu().numpy().astype(np.float64), want), pl.where(out[1].cpu().numpy(), want)


# ---- (e) error paths, the deterministic library ---------------------------------------------------------------------------
def test_error_paths():
    L = pkg()
    pl = _plan("STATIC_FEA", 0)
    sa, sb, _ = pl.desc["regions"][0]
    A, B = torch.ones(2 * sa * 32, device="cuda"), torch.ones(2 * sb * 32, device="cuda")
    pre = pl.flatten(P.int_prefill(pl.shapes), gap=-2.0)
    pl.call(A, B, 2, pre=pre)
    keep = pl.flat.clone()
    assert not np.array_equal(keep.cpu().numpy().astype(np.float64), pre)

    def raw(plan, flags, a, na, b, nb, ntiles, cnt, grads):
        rc = L.lib.rdrf_selftest_dw(plan, flags, L.ptr(a), C.c_size_t(na), L.ptr(b), C.c_size_t(nb), ntiles, L.ptr(cnt), grads,
                                    L.stream_of(pl.flat))
        torch.cuda.synchronize()
        return rc, L.lib.rdrf_last_error()

    g = C.byref(pl.struct)
    for plan in (-1, 8, 99):            # unknown plan
        rc, msg = raw(plan, 0, A, A.numel(), B, B.numel(), 2, None, g)
        assert rc == -1 and b"unknown plan" in msg
        out = (C.c_int * 64)()
        assert L.lib.rdrf_selftest_dw_describe(plan, 0, out, 64) == -1 and b"unknown plan" in L.lib.rdrf_last_error()
    out = (C.c_int * 64)()              # description buffer too small
    assert L.lib.rdrf_selftest_dw_describe(L.DW_PLANS["STATIC_FEA"], 0, out, 64) == -3
    assert b"description buffer too small" in L.lib.rdrf_last_error() and all(v == 0 for v in out)
    assert L.lib.rdrf_selftest_dw_describe(L.DW_PLANS["STATIC_FEA"], 0, None, 1 << 14) == -3
    for a, b, gr in ((None, B, g), (A, None, g), (A, B, None)):       # null rows / gradient struct
        rc, msg = raw(1, 0, a, A.numel(), b, B.numel(), 2, None, gr)
        assert rc == -1 and b"bad arguments" in msg
    rc, msg = raw(1, 0, A, A.numel(), B, B.numel(), -1, None, g)
    assert rc == -1 and b"bad arguments" in msg
    rc, msg = raw(1, 0, A, A.numel() - 1, B, B.numel(), 2, None, g)   # rows shorter than the tiles named
    assert rc == -3 and b"rows too small" in msg
    rc, msg = raw(1, 0, A, A.numel(), B, B.numel(), 3, None, g)
    assert rc == -3 and b"rows too small" in msg
    cnt = torch.tensor([65], dtype=torch.int32, device="cuda")         # a device count past the rows
    rc, msg = raw(1, 0, A, A.numel(), B, B.numel(), 2, cnt, g)
    assert rc == -1 and b"does not fit" in msg
    rc, msg = raw(1, 0, A[1:], A.numel() - 1, B, B.numel(), 1, None, g)
    assert rc == -1 and b"aligned" in msg
    # no tile: a no-op whatever the pointers; a count nobody reads does not change that
    assert raw(1, 0, None, 0, None, 0, 0, None, None)[0] == 0
    assert raw(L.DW_PLANS["SCENE_FLOW"], 0, None, 0, None, 0, 0, cnt, None)[0] == 0
    assert torch.equal(pl.flat, keep), "a refused call wrote gradients"


_DET_SIZES = [(257, None), (513, None), (32 * 256 + 1, "count")]   # odd and even tiles per workgroup; a ragged count


def _det_case(plan, flags, size, kind):
    pl = _plan(plan, flags)
    if kind == "count":
        return _exact(pl, (size + 31) // 32 + 1, size, what=f"count = {size}")
    return _exact(pl, size, what=f"ntiles = {size}")


def test_same_bits_in_the_deterministic_library(tmp_path):
    """librodynrf_det.so in a child process (the library is chosen at import), its gradient buffer bound to a fixed-point
    shadow as the fields bind theirs: after the fold, the int64 sums again, bit for bit"""
    assert run_twin(tmp_path, [CHILD, "dw"], det=True) == 2 * len(P.PLANS) + len(P.COUNT_PLANS)
