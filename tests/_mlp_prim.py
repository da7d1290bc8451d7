"""Shared by test_mlp_primitives_cpu.py and test_gpu_mlp_primitives.py: the instantiations rdrf_selftest_layer offers, the
test inputs, the error metric, the sequential-fp32 yardstick and a numpy emulation of the bf16 x 3 split
(csrc/rdrf_common.hpp split3 / mfma_seg_b3: three truncated 8-bit pieces per fp32 value, six piece products).

Every layer is seen as y[M][n_out] = X[M][n_in] @ Weff[n_out][n_in]^T: Weff = w for the forward forms, w^T for the transposed
(backward-data) forms, where w[OUT][K] is the torch.nn.Linear weight the library call takes."""
import numpy as np

F32 = np.float32

# (form, K, OUT): every (primitive, template arguments) pair the product kernels instantiate (include/rodynrf.h)
INSTANCES = [
    ("F32", 64, 64), ("F32", 128, 128), ("F32", 72, 32),
    ("F32_T", 64, 64), ("F32_T", 32, 128),
    ("B3", 144, 64), ("B3", 64, 64),
    ("B3_T", 64, 64),
    ("B3_PAIR_T", 160, 64), ("B3_PAIR_T", 96, 64),
    ("B3S", 112, 128), ("B3S", 160, 128),
    ("B3S_T", 224, 32), ("B3S_T", 96, 32), ("B3S_T", 128, 128), ("B3S_T", 96, 128), ("B3S_T", 160, 128),
]
B3_INSTANCES = [i for i in INSTANCES if i[0].startswith("B3")]
RAGGED = (1, 31, 33, 77)

# bound of the one-hot sweep, relative to |x w|: the three products the scheme drops (mid x lo, lo x mid, lo x lo) are below
# 2 * 2^-22 + 2^-30 < 2^-20 with truncated 8-bit pieces (|mid| < 2^-7 |v|, |lo| < 2^-15 |v|); six fp32 additions add 6 * 2^-24
ONE_HOT_BOUND = 2.0 ** -20 + 6 * 2.0 ** -24
# two non-zero elements per row, in different K = 16 steps: the same truncation part, twelve fp32 additions (six per step),
# each rounding at most 2^-24 of a partial sum that sum |x w| bounds
TWO_HOT_BOUND = 2.0 ** -20 + 12 * 2.0 ** -24

PRODUCTS = (("hi", "hi"), ("mid", "hi"), ("lo", "hi"), ("hi", "mid"), ("mid", "mid"), ("hi", "lo"))   # (weight piece, input piece)
REDUCED = PRODUCTS[1:]   # the five variants that lose one product (without hi x hi nothing is left to compare)


def transposed(form):
    return form.endswith("_T")


def dims(form, K, OUT):
    """(n_in, n_out) of the call"""
    return (OUT, K) if transposed(form) else (K, OUT)


def weff(form, w):
    return np.ascontiguousarray(w.T) if transposed(form) else w


def dense_inputs(form, K, OUT, M, family, seed):
    """family 'normal': standard normal rows; 'wide': normal times 10 ** randint(-3, 3) per element.  Weights normal / sqrt(K)."""
    rng = np.random.default_rng(seed)
    n_in, _ = dims(form, K, OUT)
    x = rng.standard_normal((M, n_in), dtype=F32)
    if family == "wide":
        x *= (10.0 ** np.arange(-3, 4)).astype(F32)[rng.integers(0, 7, size=(M, n_in), dtype=np.int8)]
    else:
        assert family == "normal"
    w = (rng.standard_normal((OUT, K), dtype=F32) / F32(np.sqrt(K))).astype(F32)
    return x, w


def all_ones(rng, shape):
    """fp32 values with an all-ones significand (every one of the three pieces as large as it can be), random sign, exponent
    2^-6 .. 2^6"""
    e = rng.integers(-6, 6, size=shape, endpoint=True).astype(np.uint32) + np.uint32(127)
    s = rng.integers(0, 2, size=shape).astype(np.uint32)
    return ((s << np.uint32(31)) | (e << np.uint32(23)) | np.uint32(0x007fffff)).view(F32)


def one_hot_inputs(form, K, OUT, seed, second=False):
    """M = n_in rows; row k is zero except element k (second: except elements (k + 7) % n_in and k)"""
    rng = np.random.default_rng(seed)
    n_in, _ = dims(form, K, OUT)
    v = all_ones(rng, (n_in,))
    x = np.zeros((n_in, n_in), dtype=F32)
    x[np.arange(n_in), np.arange(n_in)] = v
    if second:
        x[np.arange(n_in), (np.arange(n_in) + 7) % n_in] = all_ones(rng, (n_in,))
    w = all_ones(rng, (OUT, K))
    return x, w


def ref64(x, We, chunk=1 << 16):
    """(y64, denom): float64 product and sum_k |x_k| |w_ok|, in row chunks"""
    W64, A64 = We.astype(np.float64).T.copy(), np.abs(We).astype(np.float64).T.copy()
    y = np.empty((x.shape[0], We.shape[0]), dtype=np.float64)
    d = np.empty_like(y)
    for r0 in range(0, x.shape[0], chunk):
        xc = x[r0:r0 + chunk].astype(np.float64)
        y[r0:r0 + chunk] = xc @ W64
        d[r0:r0 + chunk] = np.abs(xc) @ A64
    return y, d


def metric(y, y64, denom):
    """e = max over the outputs of |y - y64| / sum_k |x_k| |w_ok| (outputs whose denominator is 0 must be exactly 0)"""
    err = np.abs(y.astype(np.float64) - y64)
    if (err[denom == 0] != 0).any():
        return float("inf")
    return float((err / np.where(denom == 0, 1.0, denom)).max())


def seq32(x, We):
    """plain float32 evaluation: every product rounded to fp32, accumulated sequentially in k (no BLAS, no fma)"""
    acc = np.zeros((x.shape[0], We.shape[0]), dtype=F32)
    for k in range(x.shape[1]):
        acc = acc + x[:, k:k + 1] * We[None, :, k]
    assert acc.dtype == F32
    return acc


def e_seq32(x, We, rows=4096):
    xs = x[:rows]
    y64, d = ref64(xs, We)
    return metric(seq32(xs, We), y64, d)


def split3(v):
    """csrc/rdrf_common.hpp split3: hi = top 16 bits, mid = top 16 bits of v - hi (exact), lo = top 16 bits of the rest"""
    v = np.ascontiguousarray(v, dtype=F32)
    hi = (v.view(np.uint32) & np.uint32(0xffff0000)).view(F32)
    r = v - hi
    mid = (r.view(np.uint32) & np.uint32(0xffff0000)).view(F32)
    lo = ((r - mid).view(np.uint32) & np.uint32(0xffff0000)).view(F32)
    return {"hi": hi, "mid": mid, "lo": lo}


def emulate_b3(x, We, products=PRODUCTS):
    """the piece products of the bf16 x 3 scheme summed in float64: the truncation part of its error only (the hardware adds
    its fp32 accumulation)"""
    xp = {k: p.astype(np.float64) for k, p in split3(x).items()}
    wp = {k: p.astype(np.float64).T.copy() for k, p in split3(We).items()}
    y = np.zeros((x.shape[0], We.shape[0]), dtype=np.float64)
    for pw, px in products:
        y += xp[px] @ wp[pw]
    return y
