"""Reference and inputs for stand-alone tests of the dW products (rdrf_selftest_dw; tests/test_dw_primitives_cpu.py).

rdrf_selftest_dw_describe gives a plan's job list in resolved form (include/rodynrf.h); everything here is built from that
description alone -- no row layout, no segment map.  For every job, out row r and block column c >= 0:

    dW[r - out_row0][c] += sum_tiles sum_32 A[t][A_row0 + r][s] * B[t][row0 + e][s]     for 0 <= r - out_row0 < out_dim
    db[r - out_row0]    += sum_tiles sum_32 A[t][A_row0 + r][s]

in float64 (numpy): on integer rows every term and every partial sum is an integer far below 2^53, so the float64 sums ARE
the int64 sums, and they are compared as int64."""
import ctypes as C

import numpy as np

# (plan, flags) of every job list the product builds.  Flags: 1 live_d, 2 live_b, 4 small_in_kernel (density phase)
DENSITY_FLAGS = [0, 1, 2, 3, 4, 5, 6, 7]
PLANS = [("DENSITY", 3), ("STATIC_FEA", 0), ("STATIC_TE", 0), ("DYN_APP", 0), ("DYN", 7), ("SCENE_FLOW", 0), ("FEAT_STATIC", 0),
         ("FEAT_DYN", 3)]
PLAN_IDS = [f"{p}-{f}" for p, f in PLANS]
COUNT_PLANS = [(p, f) for p, f in PLANS if p in ("STATIC_FEA", "STATIC_TE", "DYN_APP", "DYN")]
HOST_TILES = [1, 2, 3, 255, 256, 257, 512, 513, 769]
COUNTS = [0, 1, 16, 17, 31, 32, 33, 32 * 256 - 1, 32 * 256 + 1, 32 * 513 - 15]
MAXV, PREFILL = 4, 3     # |row entries| <= 4, |pre-filled gradient entries| <= 3


def partial_sum_bound(ntiles):
    """largest |partial sum| any order of accumulation can reach: the pre-fill plus 32 ntiles products of two entries"""
    return PREFILL + ntiles * 32 * MAXV * MAXV


def parse(d):
    """ints of rdrf_selftest_dw_describe -> {"dynamic", "regions": [(A_stride, B_stride, uses_count)], "jobs": [...]}"""
    d = [int(v) for v in d]
    total, nreg, njobs, dynamic = d[0:4]
    n = 4
    regions = []
    for _ in range(nreg):
        regions.append(tuple(d[n:n + 3]))
        n += 3
    jobs = []
    for _ in range(njobs):
        reg, A_row0, nbo, out_dim, out_row0, in_dim, ld, w_off, b_off, nblk = d[n:n + 10]
        n += 10
        blocks = []
        for _ in range(nblk):
            blocks.append((d[n], np.array(d[n + 1:n + 33], dtype=np.int64)))
            n += 33
        jobs.append(dict(region=reg, A_row0=A_row0, nbo=nbo, out_dim=out_dim, out_row0=out_row0, in_dim=in_dim, ld=ld, w_off=w_off,
                         b_off=b_off, blocks=blocks))
    assert n == total == len(d), (n, total, len(d))
    return dict(dynamic=bool(dynamic), regions=regions, jobs=jobs)


def describe(L, plan, flags, cap=1 << 14):
    out = (C.c_int * cap)()
    n = L.lib.rdrf_selftest_dw_describe(L.DW_PLANS[plan], flags, out, cap)
    L.check(0 if n > 0 else n, f"rdrf_selftest_dw_describe {plan} {flags}")
    return parse(out[:n])


def field_names(struct):
    """byte offset of every pointer field of a ctypes parameter struct -> name (sfw / sfb: one per element)"""
    names = {}
    for name, typ in struct._fields_:
        off = getattr(struct, name).offset
        if typ is C.c_void_p:
            names[off] = name
        elif isinstance(typ, type) and issubclass(typ, C.Array) and typ._type_ is C.c_void_p:
            for i in range(typ._length_):
                names[off + 8 * i] = f"{name}[{i}]"
    return names


def param_shapes(desc, extra_rows=2):
    """offset -> shape of the tensor behind every gradient pointer of the plan: (out_dim + extra_rows, ld) / (out_dim +
    extra_rows,); the extra rows are nobody's and must keep their pre-fill"""
    shapes = {}
    for j in desc["jobs"]:
        for off, shp in ((j["w_off"], (j["out_dim"] + extra_rows, j["ld"])), (j["b_off"], (j["out_dim"] + extra_rows,))):
            if off >= 0:
                assert shapes.setdefault(off, shp) == shp, "two jobs disagree about a parameter's shape"
    return shapes


def job_products(desc):
    """every (job, out block, input block) triple of the plan"""
    return [(ji, bo, k) for ji, j in enumerate(desc["jobs"]) for bo in range(j["nbo"]) for k in range(len(j["blocks"]))]


def reference(desc, A, B, tiles, pre, absolute=False):
    """A, B: per region [ntiles][stride][32] arrays; tiles: per region, the number of tiles that count; pre: offset -> array
    the gradients are added into.  Returns offset -> float64 array.  absolute: sum |A| |B| instead (the error metric's scale)"""
    out = {off: np.array(p, dtype=np.float64) for off, p in pre.items()}
    for j in desc["jobs"]:
        g, T = j["region"], tiles[j["region"]]
        rows = 32 * j["nbo"]
        Am = A[g][:T, j["A_row0"]:j["A_row0"] + rows].astype(np.float64)
        Am = np.abs(Am) if absolute else Am
        Am = Am.transpose(1, 0, 2).reshape(rows, T * 32)
        orow = np.arange(rows) - j["out_row0"]
        ok = (orow >= 0) & (orow < j["out_dim"])
        brows = np.concatenate([row0 + np.arange(32) for row0, _ in j["blocks"]])
        Bm = B[g][:T][:, brows].astype(np.float64)
        Bm = np.abs(Bm) if absolute else Bm
        Pall = Am @ Bm.transpose(0, 2, 1).reshape(T * 32, len(brows))     # [rows][32 per block]
        for k, (row0, cols) in enumerate(j["blocks"]):
            e = np.nonzero(cols >= 0)[0]
            np.add.at(out[j["w_off"]], (orow[ok][:, None], cols[e][None, :]), Pall[ok][:, 32 * k + e])
        if j["b_off"] >= 0:
            np.add.at(out[j["b_off"]], orow[ok], Am.sum(axis=1)[ok])
    return out


def reference_loops(desc, A, B, tiles, pre):
    """the same sums as a plain loop over every index (tiny descriptions only)"""
    out = {off: np.array(p, dtype=np.float64) for off, p in pre.items()}
    for j in desc["jobs"]:
        g = j["region"]
        for r in range(32 * j["nbo"]):
            o = r - j["out_row0"]
            if not 0 <= o < j["out_dim"]:
                continue
            for t in range(tiles[g]):
                for s in range(32):
                    a = float(A[g][t][j["A_row0"] + r][s])
                    if j["b_off"] >= 0:
                        out[j["b_off"]][o] += a
                    for row0, cols in j["blocks"]:
                        for e in range(32):
                            if cols[e] >= 0:
                                out[j["w_off"]][o][cols[e]] += a * float(B[g][t][row0 + e][s])
    return out


_POOL = {}


def int_rows(src, region, stride, ntiles, max_tiles=HOST_TILES[-1]):
    """integer rows in [-4, 4], [ntiles][stride][32] int8: every 32-row block (source, region, block index) has its own seeded
    stream, so no two staged blocks hold the same numbers and swapped blocks cannot cancel.  Generated once at the largest tile
    count and sliced (the first tiles of a longer array are the shorter array)."""
    nblk = (stride + 31) // 32
    key = (src, region, nblk)
    if key not in _POOL or _POOL[key].shape[0] < max(ntiles, max_tiles):
        T = max(ntiles, max_tiles)
        pool = np.empty((T, nblk * 32, 32), dtype=np.int8)
        for b in range(nblk):
            rng = np.random.default_rng([17, src, region, b])
            pool[:, 32 * b:32 * b + 32] = rng.integers(-MAXV, MAXV + 1, size=(T, 32, 32), dtype=np.int8)
        _POOL[key] = pool
    return _POOL[key][:ntiles, :stride]


def int_prefill(shapes, seed=5):
    return {off: np.random.default_rng([seed, off]).integers(-PREFILL, PREFILL + 1, size=shp).astype(np.float32)
            for off, shp in shapes.items()}


def ones_significand(rng, shape, bits=11):
    """integers +-(2^k - 1), 1 <= k <= bits: all-ones significands.  The product of two of them has at most 2 bits = 22
    significant bits, exact in fp32; a sum of four such products stays below 2^24 and is exact in any order"""
    k = rng.integers(1, bits + 1, size=shape)
    sign = rng.integers(0, 2, size=shape) * 2 - 1
    return (sign * (2.0 ** k - 1.0)).astype(np.float32)
