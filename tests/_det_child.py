"""The one child program of the twin-process tests (tests/_twin.py starts it).  The library is chosen when robust-dynrf_amd._lib is
imported, so a test that compares two libraries runs the other one in a process of its own: librodynrf_det.so with
RDRF_DETERMINISTIC=1, which this program then asserts it got, or whatever RDRF_LIB names.  Every mode saves its result to OUT
with torch.save:

    python tests/_det_child.py case MODULE [FUNC [ARG ...]] OUT   MODULE.FUNC(*ARGS) (default det_case); tensors go to the CPU, numpy arrays become tensors, at any depth
    python tests/_det_child.py dw OUT       tests/test_gpu_dw_primitives.py: the exact-integer cases of _DET_SIZES against
                                            librodynrf_det.so, the gradient buffer bound to a fixed-point shadow as the fields
                                            bind theirs; the number of cases that ran
    python tests/_det_child.py dw_runs OUT  tests/test_gpu_dw_runs.py: DET_CASE, the gradient buffer bound the same way
    python tests/_det_child.py scatter OUT  tests/test_gpu_scatter_primitives.py: det_cases(), every call's flat output buffer bound
                                            to a shadow; the planes and lines must not move before the fold
    python tests/_det_child.py poison OUT   tests/test_gpu_poisoned_scratch.py: every case, bit for bit per tensor"""
import ctypes as C
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _bound_call(L, pl):
    """pl.call with the flat gradient buffer bound to a shadow; folds the shadow before it returns"""
    call = pl.call
    slot = 1 if pl.desc["dynamic"] else 0
    shadow = torch.zeros(pl.total, dtype=torch.int64, device="cuda")

    def bound(A, B, ntiles, count=None, pre=None, check=True):
        pre32 = torch.from_numpy(pre).float()
        pl.flat.copy_(pre32)
        shadow.zero_()
        L.check(L.lib.rdrf_det_bind(slot, L.ptr(pl.flat), C.c_size_t(pl.total), L.ptr(shadow), L.stream_of(pl.flat)), "rdrf_det_bind")
        rc, _ = call(A, B, ntiles, count, None, check)
        assert torch.equal(pl.flat.cpu(), pre32), "an addition missed the shadow"
        L.check(L.lib.rdrf_det_finish(slot, L.stream_of(pl.flat)), "rdrf_det_finish")
        torch.cuda.synchronize()
        return rc, pl.flat
    return bound


def dw(L):
    import _dw_prim as P
    import test_gpu_dw_primitives as T
    n = 0
    for plan, flags in P.PLANS:
        pl = T._plan(plan, flags)
        pl.call = _bound_call(L, pl)
        for size, kind in T._DET_SIZES:
            if kind is None or (plan, flags) in P.COUNT_PLANS:
                T._det_case(plan, flags, size, kind)
                n += 1
    return n


class _ScatterBinder:
    """Dev.call hooks of tests/test_gpu_scatter_primitives.py: bind the flat buffer before the call, fold the shadow after it"""

    def __init__(self, L):
        self.L = L

    def bind(self, dev):
        L = self.L
        self.slot = 1 if dev.d["xw"] else 0          # dynamic / static field
        self.shadow = torch.zeros(dev.total, dtype=torch.int64, device="cuda")
        self.before = dev.flat.clone()
        L.check(L.lib.rdrf_det_bind(self.slot, L.ptr(dev.flat), C.c_size_t(dev.total), L.ptr(self.shadow), L.stream_of(dev.flat)), "rdrf_det_bind")
        # the other slot may still name the buffers of an earlier case, freed since: bind it to an empty range
        L.check(L.lib.rdrf_det_bind(1 - self.slot, L.ptr(dev.flat), C.c_size_t(0), L.ptr(self.shadow), L.stream_of(dev.flat)), "rdrf_det_bind")

    def finish(self, dev):
        L = self.L
        for k, sl in dev.slices.items():             # (dxw and g_xyz are plain stores of the sample's owner: no additions)
            if k[0] in ("plane", "line"):
                assert torch.equal(dev.flat[sl], self.before[sl]), f"{k}: an addition missed the shadow"
        assert bool((self.shadow != 0).any()) or not bool((dev.flat != self.before).any())
        L.check(L.lib.rdrf_det_finish(self.slot, L.stream_of(dev.flat)), "rdrf_det_finish")
        torch.cuda.synchronize()


def scatter(L):
    import test_gpu_scatter_primitives as T
    T.DET = _ScatterBinder(L)
    return T.det_cases()


def poison(L):
    import test_gpu_poisoned_scratch as T
    for case in T.CASES:
        T.test_fields_on_poisoned_scratch(*case)
    st, dy = T._fields("ndc")
    with T.scratch_fill(0xFF):
        p = T.run_features(st, dy)
    with T.scratch_fill(0x00):
        a = T.run_features(st, dy)
    T._finite(p, "features")
    T._compare(p, a, a, "features")
    return len(T.CASES) + 1


def dw_runs(L):
    import test_gpu_dw_primitives as T
    import test_gpu_dw_runs as R
    plan, flags, ntiles = R.DET_CASE
    pl = T._plan(plan, flags)
    pl.call = _bound_call(L, pl)
    R.exact_with_nan_elsewhere(pl, ntiles)
    return 1


def _to_cpu(v):
    if isinstance(v, torch.Tensor):
        return v.detach().cpu()
    if isinstance(v, (np.ndarray, np.generic)):
        return torch.from_numpy(np.asarray(v))
    if isinstance(v, dict):
        return {k: _to_cpu(x) for k, x in v.items()}
    return type(v)(_to_cpu(x) for x in v) if isinstance(v, (list, tuple)) else v


def case(L, module, func="det_case", *args):
    return _to_cpu(getattr(importlib.import_module(module), func)(*args))


if __name__ == "__main__":
    L = importlib.import_module("robust-dynrf_amd._lib")
    if os.environ.get("RDRF_DETERMINISTIC") == "1":
        assert L.DETERMINISTIC and L.lib.rdrf_deterministic() == 1
    mode, *args, out = sys.argv[1:]
    torch.save({"case": case, "dw": dw, "dw_runs": dw_runs, "scatter": scatter, "poison": poison}[mode](L, *args), out)
