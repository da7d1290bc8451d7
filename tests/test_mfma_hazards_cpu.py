"""Lint of the instruction stream around the bf16 MFMAs (tools/mfma_hazards.py; hipcc cross-compiles gfx950 without a GPU).
The bf16 x 3 layers are kept right by instruction ORDER (csrc/rdrf_common.hpp: "loads first", "hi, mid, lo", the scheduling
barriers), which a compiler update may undo without any numerical test noticing: the faults it cured were one stale piece in
some 15 000 samples, 1e-5 relative.  Per kernel, inside basic blocks: RAW distance = instructions between the last VALU write
of an MFMA's A / B operand and the MFMA, WAR distance = instructions between the MFMA and the next VALU write of its A / B
operand.

What the lint found when it was first run, on the build before it existed (profiles/r09_mfma_hazards_parent.txt): 133 bf16
MFMAs of the product kernels with a VALU write of an operand register 0 .. 2 instructions behind them -- 2 is the distance at
which csrc/rdrf_common.hpp records stale pieces in the fused render kernel:
  rdrf_fwd  120 at WAR distance 0, all on the A operand (weight fragment), k_static_app x 4 and k_dyn_app x 2: the `v_or_b32`
            that forms the LDS address (beyond the 64 KB an offset field reaches) of the NEXT fragment's ds_read_b128, allocated to
            the first register of the fragment just consumed; 4 more of the same kind (`v_add_u32`) in k_dyn_density_bwd.
  rdrf_bwd  9 of k_dyn_density_bwd at distance 0 .. 2 on A and B: the caller's pointer arithmetic right after the last MFMA
            of a layer.
Cured in csrc/rdrf_common.hpp (lds_frag_base: one opaque lane base per image, immediate offsets, so that no address is formed
between the MFMAs; mfma_tail_pad: three wait states behind the last MFMA of a step; scheduling barriers between the hi / mid / lo
sweeps of the split).  Figures of the current tree (profiles/r09_mfma_hazards.txt): 9972 bf16 MFMAs, 0 unchecked; min WAR 3
(k_dyn_density_bwd), min RAW 6; every kernel at or above its line of the parent table."""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENT_TABLE = os.path.join(ROOT, "profiles", "r09_mfma_hazards_parent.txt")

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("c++filt") is None, reason="needs hipcc")

# six MFMAs per 32-neuron output block and K = 16 step (hi / mid / lo pieces): what the source implies per kernel.
# (token of the mangled name, tokens that exclude, minimum per kernel, kernels at least)
FAMILIES = {
    "rdrf_fwd": [("k_static_app", ("bwd",), 4 * 18 * 6, 4),                 # (16 + 64 + 64) / 8 steps, four blocks
                 ("k_dyn_app", ("bwd",), 4 * 15 * 6, 2),                    # (16 + 32 + 8 + 64) / 8 steps
                 ("k_dyn_density", ("bwd",), 2 * 2 * 9 * 6, 5)],            # two heads x mfma_seg_b3<2, 72>
    "rdrf_bwd": [("k_static_app_bwd", (), 3 * 2 * 6, 3),                    # features only: <3, 16>; full: + <4, 64> + <5, 64>
                 ("k_dyn_app_bwd", (), 7 * 2 * 6, 3),                       # features only: <7, 16>; full: + <4, 64> + <3, 64>
                 ("k_dyn_density_bwd", (), (2 + 3) * 4 * 6, 6)],            # warp: b3<2, 32> + pair<2, 1, 32>; heads: 2 x pair<3, 2, 32>
    "rdrf_bwd_fused": [("k_dyn_warp_bwd_dw", (), (2 + 1) * 4 * 6, 2)],     # b3<2, 32> + pair<2, 1, 32>, whose two X0 blocks are dead without g_xyz
    "rdrf_render": [("k_render_fused", (), 4 * 18 * 6 + 2 * 2 * 9 * 6 + 4 * 15 * 6, 2)],
    "rdrf_selftest": [("k_st_b3s_chain", (), 4 * 7 * 6, 2), ("k_st_b3s_t", (), 3 * 2 * 6, 5),
                      ("k_st_b3_pair", (), 3 * 4 * 6, 2), ("k_st_b3I", (), 2 * 4 * 6, 2)],
}
UNIT_TOTALS = {"rdrf_fwd": 3528, "rdrf_bwd": 2976, "rdrf_bwd_fused": 120 + 72, "rdrf_render": 2016, "rdrf_motion": 0,   # rdrf_motion: the scene-flow MLP is fp32
               "rdrf_selftest": 108 + 48 + 120 + 72 + 168 + 240 + 84 + 36 + 192 + 144 + 240}


@pytest.fixture(scope="module")
def lint():
    spec = importlib.util.spec_from_file_location("mfma_hazards", os.path.join(ROOT, "tools", "mfma_hazards.py"))
    H = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(H)
    results = H.run()
    total = sum(r["n"] for _, k, r in results if k)
    unchecked = sum(len(r["unchecked"]) for _, k, r in results if k)
    print(f"\n{total} bf16 MFMAs, {unchecked} unchecked ({100.0 * unchecked / max(total, 1):.2f} %)")
    for line in H.table_lines(results):
        print(line)
    return H, results


def test_every_bf16_mfma_is_seen_and_parsed(lint):
    """a renamed mnemonic or an operand form the parser does not read cannot empty the check"""
    H, results = lint
    assert {u for u, _, _ in results} == set(UNIT_TOTALS)
    for unit, want in UNIT_TOTALS.items():
        got = sum(r["n"] for u, k, r in results if u == unit and k)
        assert got >= want, (unit, got, want)
        for token, exclude, per_kernel, kernels in FAMILIES.get(unit, ()):
            fam = [(k, r) for u, k, r in results if u == unit and k and token in k and not any(x in k for x in exclude)]
            assert len(fam) >= kernels, (unit, token, [k for k, _ in fam])
            for k, r in fam:
                assert r["n"] >= per_kernel, (k, r["n"], per_kernel)
    for unit, k, r in results:
        if k:
            for u in r["unchecked"]:
                print("unchecked:", unit, k, u)
            assert len(r["unchecked"]) <= 0.05 * r["n"], (k, len(r["unchecked"]), r["n"])
            assert len(r["raw"]) + len(r["unchecked"]) == r["n"]


def test_distances_not_below_the_parent_build(lint):
    """no kernel's minimum RAW or WAR distance falls below what the parent build shows with the same tool (the build the
    repeated-run experiments validated); kernels the parent did not have stay within the range of its kernels"""
    H, results = lint
    parent = H.read_table(PARENT_TABLE)
    assert len(parent) >= 26   # 25 kernels with bf16 MFMAs and the unit without
    floor_raw = min(v[2] for v in parent.values())
    seen = set()
    for unit, k, r in results:
        if not k:
            assert UNIT_TOTALS[unit] == 0, unit
            continue
        raw, war = min(r["raw"], default=H.NONE), min(r["war"], default=H.NONE)
        if (unit, k) in parent:
            seen.add((unit, k))
            n, _, praw, pwar = parent[(unit, k)]
            assert r["n"] >= n, (k, r["n"], n)
            assert raw >= praw, f"{k}: min RAW distance {raw} < {praw} of the parent build"
            assert war >= pwar, f"{k}: min WAR distance {war} < {pwar} of the parent build"
        else:
            assert unit == "rdrf_selftest", f"{unit} {k}: not in {os.path.basename(PARENT_TABLE)}"
            assert raw >= floor_raw, f"{k}: min RAW distance {raw} < {floor_raw}, the smallest of the parent build"
            assert war > 2, f"{k}: min WAR distance {war}"
    missing = [key for key in parent if key[1] != "-" and key not in seen]
    assert not missing, f"kernels of the parent table that the build no longer has (regenerate the table with its recipe): {missing}"


def test_war_distance_above_two_everywhere(lint):
    """2 is the distance csrc/rdrf_common.hpp documents as having returned stale operands"""
    H, results = lint
    bad = {}
    for unit, k, r in results:
        if k:
            n = sum(1 for d in r["war"] if d <= 2)
            if n:
                bad[f"{unit} {k}"] = (n, min(r["war"]))
    assert not bad, "bf16 MFMAs whose A / B operand a VALU instruction overwrites within two instructions (count, min): " + str(bad)
