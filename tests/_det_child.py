"""Child program of the deterministic-library checks (the library is chosen when robust-dynrf_amd._lib is imported, so they run
in a process of their own with RDRF_DETERMINISTIC=1):

    python tests/_det_child.py dw OUT       tests/test_gpu_dw_primitives.py: the exact-integer cases of _DET_SIZES against
                                            librodynrf_det.so, the gradient buffer bound to a fixed-point shadow as the fields
                                            bind theirs; writes the number of cases that ran to OUT
    python tests/_det_child.py scatter OUT  tests/test_gpu_scatter_primitives.py: det_cases(), every call's flat output buffer bound
                                            to a shadow; the planes and lines must not move before the fold
    python tests/_det_child.py poison OUT   tests/test_gpu_poisoned_scratch.py: every case, bit for bit per tensor"""
import ctypes as C
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

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


if __name__ == "__main__":
    L = importlib.import_module("robust-dynrf_amd._lib")
    assert L.DETERMINISTIC and L.lib.rdrf_deterministic() == 1
    n = {"dw": dw, "scatter": scatter, "poison": poison}[sys.argv[1]](L)
    with open(sys.argv[2], "w") as f:
        f.write(str(n))
