"""Child program of tests/test_gpu_dw_runs.py::test_same_bits_in_the_deterministic_library (the library is chosen when
robust-dynrf_amd._lib is imported, so it runs in a process of its own with RDRF_DETERMINISTIC=1):

    python tests/_dw_runs_child.py OUT      DET_CASE of that file against librodynrf_det.so, the gradient buffer bound to a
                                            fixed-point shadow as tests/_det_child.py binds it; writes the number of cases to OUT"""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402, F401

if __name__ == "__main__":
    L = importlib.import_module("robust-dynrf_amd._lib")
    assert L.DETERMINISTIC and L.lib.rdrf_deterministic() == 1
    import _det_child as D
    import test_gpu_dw_primitives as T
    import test_gpu_dw_runs as R
    plan, flags, ntiles = R.DET_CASE
    pl = T._plan(plan, flags)
    pl.call = D._bound_call(L, pl)
    R.exact_with_nan_elsewhere(pl, ntiles)
    with open(sys.argv[1], "w") as f:
        f.write("1")
