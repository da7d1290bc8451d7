"""k_dw3 on the lists the flat training path launches: the density phase with the warp MLP's (and the small layers') gradients
formed by their backward-data kernels.  Those plans stage up to four runs of consecutive rows and nothing between them, and the
ones whose waves hold at most two products run the 2-set instantiation, two workgroups to a CU (grid 512).

Method of tests/test_gpu_dw_primitives.py (a) and (b): integer rows in [-4, 4], integer pre-fill, torch.equal against the int64
sums built from rdrf_selftest_dw_describe alone (tests/_dw_prim.py).  Every row that is an operand of no product -- T, H3, H4, HD,
HB and the dz rows no job names: what used to be staged as bridges -- holds NaN: a plan that stages one of them and multiplies it,
or addresses a run one block off, cannot stay bit-equal.  Tile counts give a workgroup 0, 1, 2 or 3 tiles at grids of 256 and of
512 and both buffer parities at loop exit."""

import numpy as np
import pytest
import torch

import _dw_prim as P
import test_gpu_dw_primitives as T

from _twin import CHILD, run_twin

pytestmark = pytest.mark.gpu

RUN_PLANS = [("DENSITY", f) for f in (9, 10, 11, 13, 14, 15)] + [("DYN", 15)]
TILES = [1, 2, 3, 255, 256, 257, 511, 512, 513, 1025]
DET_CASE = ("DENSITY", 15, 513)


def operand_rows(desc, g):
    """boolean masks over the dz rows and the activation rows of region g: rows of a block that some product reads"""
    sa, sb, _ = desc["regions"][g]
    a, b = np.zeros(sa, dtype=bool), np.zeros(sb, dtype=bool)
    for j in desc["jobs"]:
        if j["region"] == g:
            a[j["A_row0"]:j["A_row0"] + 32 * j["nbo"]] = True
            for row0, _ in j["blocks"]:
                b[row0:row0 + 32] = True
    return a, b


def exact_with_nan_elsewhere(pl, ntiles):
    desc = pl.desc
    A = [P.int_rows(0, g, sa, ntiles, max_tiles=TILES[-1]) for g, (sa, _, _) in enumerate(desc["regions"])]
    B = [P.int_rows(1, g, sb, ntiles, max_tiles=TILES[-1]) for g, (_, sb, _) in enumerate(desc["regions"])]
    assert P.partial_sum_bound(ntiles) < 2 ** 24
    pre = P.int_prefill(pl.shapes)
    want = pl.flatten(P.reference(desc, A, B, [ntiles] * len(A), pre), gap=-2.0)
    assert np.abs(want).max() < 2 ** 24 and (want == np.rint(want)).all()
    Ag, Bg, poisoned = [], [], 0
    for g in range(len(A)):
        ma, mb = operand_rows(desc, g)
        a, b = torch.from_numpy(A[g]).cuda().float(), torch.from_numpy(B[g]).cuda().float()
        a[:, torch.from_numpy(~ma).cuda()] = float("nan")
        b[:, torch.from_numpy(~mb).cuda()] = float("nan")
        poisoned += int((~ma).sum()) + int((~mb).sum())
        Ag.append(a)
        Bg.append(b)
    assert poisoned >= 32, "the plan leaves no row unread: nothing to poison"
    _, got = pl.call(pl.rows(Ag), pl.rows(Bg), ntiles, None, pre=pl.flatten(pre, gap=-2.0))
    if not torch.equal(got.cpu().double(), torch.from_numpy(want)):
        pytest.fail(f"{pl.plan}-{pl.flags} ntiles = {ntiles}: {pl.where(got.cpu().numpy(), want)}")


@pytest.mark.parametrize("ntiles", TILES)
@pytest.mark.parametrize("plan,flags", RUN_PLANS, ids=[f"{p}-{f}" for p, f in RUN_PLANS])
def test_exact_integer_sums_with_nan_in_every_row_no_product_reads(plan, flags, ntiles):
    exact_with_nan_elsewhere(T._plan(plan, flags), ntiles)


@pytest.mark.parametrize("plan,flags", [("DENSITY", 15), ("DYN", 15)], ids=["DENSITY-15", "DYN-15"])
def test_one_product_at_a_time(plan, flags):
    """(b) of tests/test_gpu_dw_primitives.py on the four-run plan: a wrong run base or select names the product it breaks"""
    T.test_one_product_at_a_time(plan, flags)


def test_same_bits_in_the_deterministic_library(tmp_path):
    """librodynrf_det.so in a child process (the library is chosen at import): DET_CASE, the gradient buffer bound to a
    fixed-point shadow, gives the int64 sums bit for bit"""
    assert run_twin(tmp_path, [CHILD, "dw_runs"], det=True, timeout=300) == 1
