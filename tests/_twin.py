"""Parent side of the twin-process tests.  The library is chosen when robust-dynrf_amd._lib is imported (librodynrf_det.so through
RDRF_DETERMINISTIC=1, librodynrf_tools.so through RDRF_LIB), so a test that needs another library starts one child process
(tests/_det_child.py, or the test file's own __main__ block), loads what the child saved and compares it bit for bit."""
import functools
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "_det_child.py")
_INT_OF_WIDTH = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def run_twin(tmp_path, argv, *, det=None, lib=None, extra_env=None, keep_margins=False, timeout=600):
    """runs `python *argv OUT` once from the repository root and returns torch.load(OUT).  The child never inherits RDRF_LIB
    (lib sets it), records no margins under the parent's test id unless keep_margins, and gets RDRF_DETERMINISTIC=1 / 0 for
    det=True / False (None: as inherited); extra_env goes on top.  A child that fails fails the test: nothing is retried."""
    env = dict(os.environ)
    env.pop("RDRF_LIB", None)
    if lib is not None:
        env["RDRF_LIB"] = lib
    if not keep_margins:
        env.pop("RDRF_MARGINS", None)
    if det is not None:
        env["RDRF_DETERMINISTIC"] = "1" if det else "0"
    env.update(extra_env or {})
    out = str(tmp_path / f"twin_{len(os.listdir(tmp_path))}.pt")
    r = subprocess.run([sys.executable, *argv, out], env=env, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, f"child exited {r.returncode}\n" + r.stdout[-2000:] + r.stderr[-4000:]
    return torch.load(out)


@functools.lru_cache(maxsize=None)
def tools_lib():
    """the path of librodynrf_tools.so (the build whose environment switches are live), built first if it is missing"""
    path = os.path.join(ROOT, "robust-dynrf_amd", "librodynrf_tools.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "robust-dynrf_amd", "csrc"), "-j16", "tools"], timeout=1800)
    return path


def same_bits(a, b):
    """dtype, shape and every byte agree: a NaN equals a NaN of the same payload, +0.0 differs from -0.0"""
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    a, b = a.detach().contiguous().cpu(), b.detach().contiguous().cpu()
    if a.is_floating_point() or a.is_complex():
        if a.is_complex():
            a, b = torch.view_as_real(a), torch.view_as_real(b)
        a, b = a.view(_INT_OF_WIDTH[a.element_size()]), b.view(_INT_OF_WIDTH[b.element_size()])
    return torch.equal(a, b)


def assert_same_dict(det, ours):
    """the two flat dicts of tensors hold the same keys and, key by key, the same bits"""
    assert sorted(det) == sorted(ours), f"keys differ: {sorted(det)} vs {sorted(ours)}"
    for k in sorted(ours):
        assert same_bits(det[k], ours[k]), k
