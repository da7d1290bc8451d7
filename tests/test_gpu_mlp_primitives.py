"""Every MLP layer primitive of csrc/rdrf_common.hpp on its own (rdrf_selftest_layer: the product's template arguments, the
product's pack code, raw accumulators) against float64, in the conditioning-free metric

    e = max over the outputs of |y - y64| / sum_k |x_k| |w_ok|.

The end-to-end parity tests hold 1e-4 of max|ref|; a bf16 x 3 layer that loses one of its six piece products is wrong by
about 1.5e-5 of sum |w x| and passes them all (tests/test_mlp_primitives_cpu.py shows both numbers on a CPU emulation).

(a) dense, M = 2^20 and the ragged sizes: e <= 2 x e_seq32, the same metric of a sequential fp32 evaluation of the same inputs
    (numpy, 4096 rows).  The fp32 matrix instruction and bf16 x 3 are held to the same bound; the factor 2 covers a different
    summation order and nothing more.  A lost product sits 10 to 30 times above it.
(b) one-hot sweep with all-ones significands: every weight position and every piece of every pack mode, one by one, within
    (2^-20 + 6 * 2^-24) |x w| -- derived from the piece widths (tests/_mlp_prim.py), a factor 11 from both the six products'
    own error and a single lost product.
(c) the same bits from two calls, and from the deterministic library.
(d) error paths.

The forms do not depend on the RDRF_APP_F32 / RDRF_HEADS_F32 build switches: RDRF_LIB=<a tools/build_variant.sh library> runs
this file against such a build."""
import ctypes as C

import numpy as np
import pytest
import torch

import _mlp_prim as P
from _twin import CHILD, assert_same_dict, run_twin
from _util import pkg, profile_line, record_margin

pytestmark = pytest.mark.gpu

M_DENSE = 1 << 20
WS_BYTES = 128 << 10
CANARY = -1234.5
IDS = [f"{f}-{k}-{o}" for f, k, o in P.INSTANCES]
B3_IDS = [f"{f}-{k}-{o}" for f, k, o in P.B3_INSTANCES]


def _call(form, x, w, K, OUT, M=None, ws_bytes=WS_BYTES):
    """x: cuda [>= M][n_in], w: cuda [OUT][K] -> (rc, y [M + 32][n_out]); the 32 extra rows keep their canary"""
    L = pkg()
    n_in, n_out = P.dims(form, K, OUT)
    M = x.shape[0] if M is None else M
    assert x.shape[1] == n_in and tuple(w.shape) == (OUT, K) and x.is_contiguous() and w.is_contiguous()
    y = torch.full((M + 32, n_out), CANARY, device="cuda")
    ws = torch.empty(WS_BYTES, dtype=torch.uint8, device="cuda")
    rc = L.lib.rdrf_selftest_layer(L.SELFTEST_FORMS[form], L.ptr(x), L.ptr(w), M, K, OUT, L.ptr(y), L.ptr(ws),
                                   C.c_size_t(ws_bytes), L.stream_of(y))
    torch.cuda.synchronize()
    return rc, y


def _run(form, x, w, K, OUT, M=None):
    L = pkg()
    rc, y = _call(form, x, w, K, OUT, M)
    L.check(rc, f"selftest_layer {form} {K} -> {OUT}")
    M = x.shape[0] if M is None else M
    assert bool((y[M:] == CANARY).all()), "rows past M were written"
    return y[:M]


# ---- (a) dense accuracy ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["normal", "wide"])
@pytest.mark.parametrize("form,K,OUT", P.INSTANCES, ids=IDS)
def test_dense_accuracy_against_float64(form, K, OUT, family):
    x, w = P.dense_inputs(form, K, OUT, M_DENSE, family, seed=1000 + 2 * P.INSTANCES.index((form, K, OUT)) + (family == "wide"))
    We = P.weff(form, w)
    e32 = P.e_seq32(x, We)
    bound = 2.0 * e32
    xg, wg = torch.from_numpy(x).cuda(), torch.from_numpy(w).cuda()
    yg = _run(form, xg, wg, K, OUT)
    y = yg.cpu().numpy()
    y64, d = P.ref64(x, We)
    e = P.metric(y, y64, d)
    print(f"{form:10s} {K:3d} -> {OUT:3d} {family:6s} M = 2^20: e = {e:.3e}   e_seq32 = {e32:.3e}   e / (2 e_seq32) = {e / bound:.3f}")
    profile_line("RDRF_MLP_PRIM_TABLE", f"{form:10s} {K:4d} {OUT:4d} {family:7s} {e:.3e} {e32:.3e} {e / bound:.3f}")
    record_margin(f"{form} {K}->{OUT} {family} dense e / (2 e_seq32)", e / bound)
    worst = e
    for m in P.RAGGED:
        # a tile's columns are independent samples: the first m rows of the big call, bit for bit, and nothing past row m
        ym = _run(form, xg, wg, K, OUT, M=m)
        assert torch.equal(ym, yg[:m]), f"M = {m}: rows differ from the M = 2^20 call"
        worst = max(worst, P.metric(ym.cpu().numpy(), y64[:m], d[:m]))
    record_margin(f"{form} {K}->{OUT} {family} ragged e / (2 e_seq32)", worst / bound)
    assert worst <= bound, f"{form} {K}->{OUT} {family}: e = {worst:.3e} > 2 x e_seq32 = {bound:.3e}"


# ---- (b) one-hot sweep ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("second", [False, True], ids=["one", "two"])
@pytest.mark.parametrize("form,K,OUT", P.INSTANCES, ids=IDS)
def test_one_hot_sweep_every_weight_position(form, K, OUT, second):
    x, w = P.one_hot_inputs(form, K, OUT, seed=2000 + P.INSTANCES.index((form, K, OUT)), second=second)
    We = P.weff(form, w)
    y = _run(form, torch.from_numpy(x).cuda(), torch.from_numpy(w).cuda(), K, OUT).cpu().numpy()
    y64, d = P.ref64(x, We)
    assert (d > 0).all()
    rel = np.abs(y.astype(np.float64) - y64) / d
    bound = P.TWO_HOT_BOUND if second else P.ONE_HOT_BOUND
    k, o = np.unravel_index(np.argmax(rel), rel.shape)
    print(f"{form:10s} {K:3d} -> {OUT:3d} {'two' if second else 'one'}-hot: worst {rel.max():.3e} at input {k}, output {o}; bound {bound:.3e}")
    record_margin(f"{form} {K}->{OUT} {'two' if second else 'one'}-hot / bound", float(rel.max()) / bound)
    bad = np.argwhere(rel > bound)
    assert len(bad) == 0, (f"{form} {K}->{OUT}: {len(bad)} of {rel.size} (input, output) positions exceed {bound:.3e} |x w|; "
                           f"first {bad[:8].tolist()}, worst {rel.max():.3e}")


# ---- (c) same bits twice --------------------------------------------------------------------------------------------------
def _dense_case(form, K, OUT):
    x, w = P.dense_inputs(form, K, OUT, M_DENSE, "normal", seed=3000 + P.INSTANCES.index((form, K, OUT)))
    return torch.from_numpy(x).cuda(), torch.from_numpy(w).cuda()


@pytest.mark.parametrize("form,K,OUT", P.B3_INSTANCES, ids=B3_IDS)
def test_same_bits_twice(form, K, OUT):
    """two calls on the same inputs (no loop: a difference is a finding to diagnose, not something to re-run)"""
    xg, wg = _dense_case(form, K, OUT)
    a = _run(form, xg, wg, K, OUT)
    b = _run(form, xg, wg, K, OUT)
    if not torch.equal(a, b):
        diff = (a != b).nonzero()
        pytest.fail(f"{form} {K}->{OUT}: {len(diff)} outputs differ between two calls, first {diff[:8].tolist()}")


def det_case():
    """what both libraries compute (tests/_det_child.py case): the first 2^16 rows of every bf16 x 3 instance's dense case"""
    out = {}
    for form, K, OUT in P.B3_INSTANCES:
        xg, wg = _dense_case(form, K, OUT)
        out[f"{form}-{K}-{OUT}"] = _run(form, xg, wg, K, OUT)[:1 << 16]
    return out


def test_same_bits_in_the_deterministic_library(tmp_path):
    """librodynrf_det.so in a child process (the library is chosen at import) writes the bits of the product library"""
    out = {det: run_twin(tmp_path, [CHILD, "case", "test_gpu_mlp_primitives"], det=det, timeout=900) for det in (False, True)}
    assert sorted(out[False]) == sorted(B3_IDS)
    assert_same_dict(out[True], out[False])


# ---- (d) error paths ------------------------------------------------------------------------------------------------------
def test_error_paths():
    L = pkg()
    x = torch.randn(64, 64, device="cuda")
    w = torch.randn(64, 64, device="cuda")
    rc, y = _call("B3", x, w, 64, 64)
    assert rc == 0 and bool((y[:64] != CANARY).all())
    # unknown form
    ws = torch.empty(WS_BYTES, dtype=torch.uint8, device="cuda")
    y = torch.full((64, 64), CANARY, device="cuda")
    for form in (-1, 7, 99):
        rc = L.lib.rdrf_selftest_layer(form, L.ptr(x), L.ptr(w), 64, 64, 64, L.ptr(y), L.ptr(ws), C.c_size_t(WS_BYTES), L.stream_of(y))
        assert rc < 0 and b"unknown form" in L.lib.rdrf_last_error()
    # a (K, OUT) the form is not instantiated for
    for form, K, OUT in (("B3", 64, 128), ("B3_T", 144, 64), ("F32", 72, 64), ("B3S", 64, 64), ("B3S_T", 64, 64), ("B3S_T", 100, 32),
                         ("B3_PAIR_T", 64, 64), ("F32_T", 128, 128)):
        n_in, n_out = P.dims(form, K, OUT)
        rc = L.lib.rdrf_selftest_layer(L.SELFTEST_FORMS[form], L.ptr(x), L.ptr(w), 1, K, OUT, L.ptr(y), L.ptr(ws),
                                       C.c_size_t(WS_BYTES), L.stream_of(y))
        assert rc == -1 and b"not instantiated" in L.lib.rdrf_last_error(), (form, K, OUT)
    # short workspace
    rc, y2 = _call("B3", x, w, 64, 64, ws_bytes=2 * 32 * 96 * 4 - 16)
    assert rc < 0 and b"workspace too small" in L.lib.rdrf_last_error()
    assert bool((y2 == CANARY).all())
    # null pointers
    rc = L.lib.rdrf_selftest_layer(2, None, L.ptr(w), 64, 64, 64, L.ptr(y), L.ptr(ws), C.c_size_t(WS_BYTES), L.stream_of(y))
    assert rc < 0 and b"bad arguments" in L.lib.rdrf_last_error()
    # M = 0 is a no-op, whatever the pointers
    rc = L.lib.rdrf_selftest_layer(2, None, None, 0, 64, 64, None, None, C.c_size_t(0), L.stream_of(y))
    assert rc == 0
    torch.cuda.synchronize()
    assert bool((y == CANARY).all())
