"""Child program of tests/test_gpu_simplify.py::test_deterministic_library_gives_the_same_bits: the library is chosen when
robust-dynrf_amd._lib is imported, so the deterministic twin runs in a process of its own (RDRF_DETERMINISTIC=1).

    python tests/_simplify_det_child.py OUT     writes the meshes of test_gpu_simplify.det_case() to OUT (torch.save)"""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

if __name__ == "__main__":
    L = importlib.import_module("robust-dynrf_amd._lib")
    assert L.DETERMINISTIC and L.lib.rdrf_deterministic() == 1
    import test_gpu_simplify as T
    torch.save(T.det_case(), sys.argv[1])
