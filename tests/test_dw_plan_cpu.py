"""The host planner of the dW products on its own (rdrf_selftest_dw_plan: the launches dw_launch makes for a plan's job list, host
code only), held against the job list that rdrf_selftest_dw_describe reports.  No GPU.

For every (plan, flags) the product builds: every product's operands are staged blocks of the right source and the right rows,
every product of the job list is formed exactly once, the staged blocks are unique, the runs are consecutive rows and at most
four, at most 30 blocks, at most 4 (2 in the 2-set instantiation) products per wave, LDS = blocks x 4 KB.  On the flat training
path (density phase with the small layers and the warp MLP formed by their backward-data kernels) no block is staged that no
product reads; the two-kernel list with both heads live stages exactly one, the K1G_SM bridge."""
import ctypes as C

import pytest

import _dw_prim as P

from _util import pkg

MAX_RUNS, MAX_BLK, WAVES = 4, 30, 12
PAIRS = (P.PLANS + [("DENSITY", f) for f in P.DENSITY_FLAGS if f != 3] + [("DENSITY", f) for f in range(8, 16)]
         + [("DYN", f) for f in (13, 14, 15)])
FLAT = {13: 8, 14: 8, 15: 13}     # flat training path: staged blocks of the density-phase launch (2 dz + 3 + 3; 4 dz + 3 + 3 + 3)
NTILES = [1, 300, 511, 512, 1025]


def launches(L, plan, flags, ntiles, cap=1 << 14):
    out = (C.c_int * cap)()
    n = L.lib.rdrf_selftest_dw_plan(L.DW_PLANS[plan], flags, ntiles, out, cap)
    L.check(0 if n > 0 else n, f"rdrf_selftest_dw_plan {plan} {flags}")
    d = [int(v) for v in out[:n]]
    i, res = 2, []
    for _ in range(d[1]):
        grid, lds, nacc, nblk, nseg = d[i:i + 5]
        i += 5
        runs = [tuple(d[i + 3 * q:i + 3 * q + 3]) for q in range(nseg)]
        i += 3 * nseg
        blocks = [tuple(d[i + 2 * q:i + 2 * q + 2]) for q in range(nblk)]
        i += 2 * nblk
        waves = []
        for _w in range(WAVES):
            npr = d[i]
            i += 1
            waves.append([tuple(d[i + 5 * k:i + 5 * k + 5]) for k in range(npr)])
            i += 5 * npr
        res.append(dict(grid=grid, lds=lds, nacc=nacc, runs=runs, blocks=blocks, waves=waves))
    assert i == n == d[0]
    return res


def unused_blocks(launch):
    used = {x for w in launch["waves"] for (a, b, _, _, _) in w for x in (a, b)}
    return [blk for i, blk in enumerate(launch["blocks"]) if i not in used]


def test_symbol_is_bound():
    L = pkg()
    assert hasattr(L.lib, "rdrf_selftest_dw_plan") and "rdrf_selftest_dw_plan" in L.SYMBOLS


@pytest.mark.parametrize("ntiles", [1, 1025])
@pytest.mark.parametrize("plan,flags", PAIRS, ids=[f"{p}-{f}" for p, f in PAIRS])
def test_launches_are_well_formed_and_cover_the_job_list(plan, flags, ntiles):
    L = pkg()
    desc = P.describe(L, plan, flags)
    ls = launches(L, plan, flags, ntiles)
    formed = []
    for l in ls:
        blocks, runs = l["blocks"], l["runs"]
        assert 1 <= len(blocks) <= MAX_BLK and l["lds"] == len(blocks) * 4096
        assert len(set(blocks)) == len(blocks), "a block is staged twice"
        assert blocks == sorted(blocks)
        assert 1 <= len(runs) <= MAX_RUNS and runs[0][2] == 0
        ends = [r[2] for r in runs[1:]] + [len(blocks)]
        for (src, row0, b0), end in zip(runs, ends):      # a run: consecutive rows of one source
            assert b0 < end
            for i in range(b0, end):
                assert blocks[i] == (src, row0 + 32 * (i - b0)), (runs, blocks)
        assert l["nacc"] in (2, 4)
        assert max(len(w) for w in l["waves"]) <= l["nacc"]
        assert l["nacc"] == (2 if max(len(w) for w in l["waves"]) <= 2 else 4)
        assert 1 <= l["grid"] <= 512
        regions = set()
        for w in l["waves"]:
            for a, b, ji, bo, k in w:
                j = desc["jobs"][ji]
                assert 0 <= a < len(blocks) and 0 <= b < len(blocks)
                assert blocks[a] == (0, j["A_row0"] + 32 * bo), "the dz operand is not the job's out block"
                assert blocks[b] == (1, j["blocks"][k][0]), "the input operand is not the job's input block"
                regions.add(j["region"])
                formed.append((ji, bo, k))
        assert len(regions) == 1, "a launch mixes two row regions"
    assert sorted(formed) == sorted(P.job_products(desc)), "the launches do not form every product exactly once"


@pytest.mark.parametrize("flags", sorted(FLAT))
@pytest.mark.parametrize("plan", ["DENSITY", "DYN"])
def test_flat_training_path_stages_only_operands(plan, flags):
    L = pkg()
    for ntiles in NTILES:
        l = launches(L, plan, flags, ntiles)[-1]           # DYN: the density phase is the second region
        assert len(l["blocks"]) == FLAT[flags]
        assert unused_blocks(l) == []
        assert l["nacc"] == 2
        assert l["grid"] == (512 if ntiles >= 512 else ntiles)


@pytest.mark.parametrize("plan", ["DENSITY", "DYN"])
def test_two_kernel_list_bridges_the_one_block_hole(plan):
    L = pkg()
    l = launches(L, plan, 7, 257)[-1]
    un = unused_blocks(l)
    assert len(un) == 1 and un[0][0] == 0, un              # one dz block: K1G_SM between DZ4 and DZD
    row = un[0][1]
    assert (0, row - 32) in l["blocks"] and (0, row + 32) in l["blocks"]
    assert len(l["runs"]) == MAX_RUNS


def test_error_paths():
    L = pkg()
    out = (C.c_int * 8)()
    assert L.lib.rdrf_selftest_dw_plan(99, 0, 4, out, 8) == -1 and b"unknown plan" in L.lib.rdrf_last_error()
    assert L.lib.rdrf_selftest_dw_plan(L.DW_PLANS["DENSITY"], 15, 0, out, 8) == -1
    assert L.lib.rdrf_selftest_dw_plan(L.DW_PLANS["DENSITY"], 15, 4, out, 8) == -3
    assert b"description buffer too small" in L.lib.rdrf_last_error() and all(v == 0 for v in out)
