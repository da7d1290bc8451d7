"""The bounds of tests/test_gpu_mlp_primitives.py have teeth: a numpy emulation of the bf16 x 3 split (three truncated bf16
pieces per fp32 value, csrc/rdrf_common.hpp) passes them with all six piece products and fails them as soon as any one of the
five small products is lost -- an error of about 1.5e-5 of sum |w x|, ten times INSIDE the end-to-end tolerances of the
rest of the suite.  No GPU and no library call in the emulation; the last test checks that both libraries export the entry
point the GPU tests drive."""
import os
import subprocess

import numpy as np
import pytest

import _mlp_prim as P

from _util import pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("form,K,OUT", P.B3_INSTANCES, ids=lambda v: str(v))
def test_one_hot_bound_separates_a_lost_product(form, K, OUT):
    """bound (b): 1.31e-6 of |x w|.  Six products: ~1.2e-7.  Any single product missing: 1.5e-5 or more, at EVERY output"""
    x, w = P.one_hot_inputs(form, K, OUT, seed=11)
    We = P.weff(form, w)
    y64, d = P.ref64(x, We)
    full = P.metric(P.emulate_b3(x, We), y64, d)
    print(f"{form} {K}->{OUT}: six products {full:.3g}, bound {P.ONE_HOT_BOUND:.3g}")
    assert full <= P.ONE_HOT_BOUND / 5, full
    for lost in P.REDUCED:
        y = P.emulate_b3(x, We, [p for p in P.PRODUCTS if p != lost])
        rel = np.abs(y - y64)[d > 0] / d[d > 0]
        print(f"   without {lost}: min {rel.min():.3g} max {rel.max():.3g}")
        assert rel.min() > 5 * P.ONE_HOT_BOUND, (lost, rel.min())   # every weight position shows it, not just the worst


def test_two_hot_bound_separates_a_piece_from_the_wrong_step():
    """second sweep of (b): two non-zero elements per row.  A piece read from the other element's position (a wrong K step or
    lane) replaces a term by an unrelated value: far outside the bound"""
    form, K, OUT = "B3", 144, 64
    x, w = P.one_hot_inputs(form, K, OUT, seed=12, second=True)
    y64, d = P.ref64(x, w)
    assert P.metric(P.emulate_b3(x, w), y64, d) <= P.TWO_HOT_BOUND / 5
    xs = P.split3(x)
    wrong = dict(xs, lo=np.roll(xs["lo"], 7, axis=1))   # the lo pieces of the element seven slots away
    y = sum(wrong[px].astype(np.float64) @ P.split3(w)[pw].astype(np.float64).T for pw, px in P.PRODUCTS)
    assert P.metric(y, y64, d) > 5 * P.TWO_HOT_BOUND


@pytest.mark.parametrize("K,OUT,family", [(160, 64, "normal"), (64, 128, "normal"), (32, 64, "normal"), (160, 64, "wide")])
def test_dense_bound_separates_a_lost_product(K, OUT, family):
    """bound (a): 2 x the error of a sequential fp32 evaluation of the same inputs.  The six products sit below it, each
    reduced variant above it"""
    x, w = P.dense_inputs("B3", K, OUT, 4096, family, seed=21)
    y64, d = P.ref64(x, w)
    e32 = P.e_seq32(x, w)
    full = P.metric(P.emulate_b3(x, w), y64, d)
    print(f"{K}->{OUT} {family}: sequential fp32 {e32:.3g}, six products {full:.3g}")
    assert 1e-7 < e32 < 1e-6, e32
    assert full <= 2 * e32, (full, e32)
    for lost in P.REDUCED:
        e = P.metric(P.emulate_b3(x, w, [p for p in P.PRODUCTS if p != lost]), y64, d)
        print(f"   without {lost}: {e:.3g}")
        assert e > 2 * e32, (lost, e, e32)


def test_a_stale_piece_is_invisible_to_the_dense_bound():
    """what (a) can NOT see, and why the one-hot sweep, the same-bits test and the instruction-stream lint exist: one stale
    lo piece of one element of a K = 160 row stays far inside 2 x e_seq32"""
    x, w = P.dense_inputs("B3", 160, 64, 4096, "normal", seed=22)
    y64, d = P.ref64(x, w)
    xs, ws = P.split3(x), P.split3(w)
    xs["lo"][0, 5] = xs["lo"][1, 5]   # one sample reads the lo piece another sample left in the register
    y = sum(xs[px].astype(np.float64) @ ws[pw].astype(np.float64).T for pw, px in P.PRODUCTS)
    assert P.metric(y, y64, d) < 2 * P.e_seq32(x, w)


def test_split3_is_exact_and_truncating():
    rng = np.random.default_rng(3)
    v = np.concatenate([rng.standard_normal(10000).astype(np.float32), P.all_ones(rng, (10000,))])
    p = P.split3(v)
    rest = v.astype(np.float64) - p["hi"].astype(np.float64) - p["mid"].astype(np.float64) - p["lo"].astype(np.float64)
    assert (rest == 0).all()                                   # 8 + 8 + 8 bits: the whole fp32 significand
    assert (np.abs(p["mid"]) < 2.0 ** -7 * np.abs(v)).all() and (np.abs(p["lo"]) < 2.0 ** -15 * np.abs(v)).all()
    ones = P.all_ones(rng, (1000,))
    assert ((ones.view(np.uint32) & 0x007fffff) == 0x007fffff).all() and (np.abs(ones) < 128).all() and (np.abs(ones) > 2.0 ** -6).all()
    assert all((np.abs(q) > 0).all() for q in P.split3(ones).values())


def test_both_libraries_export_the_layer_selftest():
    L = pkg()
    assert "rdrf_selftest_layer" in L.SYMBOLS and hasattr(L.lib, "rdrf_selftest_layer")
    hdr = open(os.path.join(ROOT, "include", "rodynrf.h")).read()
    for name, value in L.SELFTEST_FORMS.items():
        assert f"#define RDRF_ST_{name} {value}\n" in hdr, name
    assert sorted({i[0] for i in P.INSTANCES}) == sorted(L.SELFTEST_FORMS)
    for so in ("librodynrf.so", "librodynrf_det.so"):
        path = os.path.join(ROOT, "robust-dynrf_amd", so)
        assert os.path.exists(path), path + " is not built"
        syms = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        assert " T rdrf_selftest_layer\n" in syms, so
