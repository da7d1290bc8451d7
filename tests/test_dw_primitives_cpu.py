"""CPU side of the stand-alone dW harness (rdrf_selftest_dw, tests/_dw_prim.py): the symbols, the job-list descriptions of every
plan, the reference builder against a plain loop, and the exactness bound of integer rows at every tile count listed."""
import ctypes as C
import os

import numpy as np
import pytest

import _dw_prim as P

from _util import pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", ["librodynrf.so", "librodynrf_det.so"])
def test_both_libraries_export_the_dw_selftest(name):
    lib = C.CDLL(os.path.join(ROOT, "robust-dynrf_amd", name))
    assert hasattr(lib, "rdrf_selftest_dw") and hasattr(lib, "rdrf_selftest_dw_describe")


def test_the_binding_lists_the_dw_selftest():
    L = pkg()
    assert "rdrf_selftest_dw" in L.SYMBOLS and "rdrf_selftest_dw_describe" in L.SYMBOLS


def _tiny_description():
    """two regions; a job with an out-row offset, a bias, columns with holes and a repeated column; a job without a bias"""
    cols0 = np.full(32, -1, dtype=np.int64)
    cols0[:5] = [4, 0, 2, -1, 2]
    cols1 = np.full(32, -1, dtype=np.int64)
    cols1[30:] = [1, 3]
    ident = np.arange(32, dtype=np.int64)
    ident[7:] = -1
    jobs = [dict(region=0, A_row0=32, nbo=2, out_dim=37, out_row0=3, in_dim=5, ld=6, w_off=8, b_off=16, blocks=[(0, cols0), (64, cols1)]),
            dict(region=1, A_row0=0, nbo=1, out_dim=2, out_row0=0, in_dim=7, ld=7, w_off=24, b_off=-1, blocks=[(32, ident)])]
    return dict(dynamic=True, regions=[(96, 96, 0), (32, 64, 1)], jobs=jobs)


def test_reference_agrees_with_a_plain_triple_loop():
    desc = _tiny_description()
    rng = np.random.default_rng(3)
    T = 3
    A = [rng.integers(-4, 5, size=(T, sa, 32)).astype(np.int8) for sa, _, _ in desc["regions"]]
    B = [rng.integers(-4, 5, size=(T, sb, 32)).astype(np.int8) for _, sb, _ in desc["regions"]]
    shapes = P.param_shapes(desc)
    assert shapes == {8: (39, 6), 16: (39,), 24: (4, 7)}
    pre = P.int_prefill(shapes)
    tiles = [T, 2]
    fast, slow = P.reference(desc, A, B, tiles, pre), P.reference_loops(desc, A, B, tiles, pre)
    for off in shapes:
        assert np.array_equal(fast[off], slow[off]), off
        assert np.array_equal(fast[off][-2:], pre[off][-2:])          # rows past out_dim keep their pre-fill
    assert np.array_equal(fast[8][:, 5], pre[8][:37 + 2, 5])          # a column no block maps to keeps its pre-fill
    assert not np.array_equal(fast[8][:37, :5], pre[8][:37, :5])
    mag = P.reference(desc, A, B, tiles, {o: np.zeros(s) for o, s in shapes.items()}, absolute=True)
    plain = P.reference(desc, A, B, tiles, {o: np.zeros(s) for o, s in shapes.items()})
    assert all((mag[o] >= np.abs(plain[o])).all() for o in shapes)


def test_parse_round_trip_of_the_product_plans():
    """the description of every plan parses to its full length; every job's rows and blocks lie inside the strides; a plan's
    parameters are fields of the struct it names"""
    L = pkg()
    seen = set()
    for plan, flags in P.PLANS + [("DENSITY", f) for f in P.DENSITY_FLAGS]:
        d = P.describe(L, plan, flags)
        names = P.field_names(L.RdrfDynamicParams if d["dynamic"] else L.RdrfStaticParams)
        assert len(d["regions"]) == (2 if plan in ("DYN", "FEAT_DYN") else 1)
        for j in d["jobs"]:
            sa, sb, _ = d["regions"][j["region"]]
            assert j["A_row0"] % 32 == 0 and j["A_row0"] + 32 * j["nbo"] <= sa
            assert 0 <= j["out_row0"] and j["out_row0"] + j["out_dim"] <= 32 * j["nbo"] and j["in_dim"] <= j["ld"]
            assert j["w_off"] in names and (j["b_off"] == -1 or j["b_off"] in names)
            for row0, cols in j["blocks"]:
                assert row0 % 32 == 0 and row0 + 32 <= sb and cols.max() < j["ld"] and cols.min() >= -1
            seen.add((d["dynamic"], names[j["w_off"]]))
        assert [u for _, _, u in d["regions"]] == {"DYN": [1, 0], "FEAT_DYN": [0, 0]}.get(plan, [int((plan, flags) in P.COUNT_PLANS)])
    assert (True, "sfw[0]") in seen and (False, "w1") in seen and (True, "bw1") in seen and (True, "basis") in seen
    L3 = [P.describe(L, "DENSITY", f) for f in (0, 3, 7)]
    assert [len(d["jobs"]) for d in L3] == [3, 7, 4]      # no live head; both heads; both heads, small layers in the kernel


def test_every_partial_sum_of_the_integer_test_is_exact():
    sizes = P.HOST_TILES + [(c + 31) // 32 + 1 for c in P.COUNTS] + [3, 257]
    assert max(sizes) == 769
    for n in sizes:
        assert P.partial_sum_bound(n) < 2 ** 24
    assert P.partial_sum_bound(769) == 3 + 769 * 32 * 16
    # (b): four products of two integers below 2^11
    assert 4 * (2 ** 11 - 1) ** 2 + P.PREFILL < 2 ** 24
    v = P.ones_significand(np.random.default_rng(0), (1000,))
    assert np.abs(v).max() <= 2047 and (np.log2(np.abs(v) + 1) % 1 == 0).all()
