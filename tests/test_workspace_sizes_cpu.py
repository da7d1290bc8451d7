"""The workspace and saved-buffer sizes of the C ABI against those of commit 6a91f93 (the parent of the change that derived the
backward workspace sizes from their carves): PARENT holds what every exported *_workspace_bytes and *_saved_bytes* function of
that commit's library returned, recorded by building it and calling the functions.

Kept sizes return exactly the table: the forward and render workspaces (rdrf_render_chunks_fwd coalesces chunks by comparing
rdrf_render_workspace_bytes with the caller's buffer, so another value would change launch shapes) and the saved buffers
(carve_saved_bwd tells a full buffer from a RDRF_SAVE_NO_APP one by its size).

Derived sizes are the end offset of the carve that consumes them (a WsCarver in measuring mode runs the layout function of the
entry point), so they cannot be too small; here they are held to be no larger than the parent's closed forms with their slack
terms, positive, whole 256-byte blocks and non-decreasing in each argument.  rdrf_features_workspace_bytes keeps its form
(rdrf_workspace_bytes(Np, 32) + a closed term that is no multiple of 256), so it is held to that form and to the parent's value
as an upper bound instead."""

import pytest

from _util import pkg

NS = [(1, 1), (1, 32), (1, 33), (33, 45), (4, 33), (512, 115), (4096, 115)]
MS = [1, 32, 33, 77, 4096]

# name[fixed leading arguments] -> {shape: bytes}
PARENT = {
    'rdrf_workspace_bytes': {(1, 1): 4371552, (1, 32): 4418688, (1, 33): 4559712, (33, 45): 14383840, (4, 33): 5339008, (512,
        115): 365636608, (4096, 115): 2895514880},
    'rdrf_forward_workspace_bytes': {(1, 1): 4198800, (1, 32): 4199296, (1, 33): 4199312, (33, 45): 4226640, (4, 33): 4201280,
        (512, 115): 5206272, (4096, 115): 12259584},
    'rdrf_render_workspace_bytes': {(1, 1): 8414145, (1, 32): 8418144, (1, 33): 8418273, (33, 45): 8615821, (4, 33): 8432004,
        (512, 115): 16173056, (4096, 115): 70488576},
    'rdrf_render_motion_workspace_bytes': {(1, 1): 8414145, (1, 32): 8418144, (1, 33): 8418273, (33, 45): 8615821, (4, 33):
        8432004, (512, 115): 16173056, (4096, 115): 70488576},
    'rdrf_selftest_warp_bwd_workspace_bytes': {(1, 1): 4195072, (1, 32): 4195072, (1, 33): 4195072, (33, 45): 4196352, (4, 33):
        4195072, (512, 115): 4253696, (4096, 115): 4665856},
    # (added after that commit: the weight images only, the same at every shape -- held to this as its upper bound)
    'rdrf_selftest_heads_bwd_workspace_bytes': {(1, 1): 4194304, (1, 32): 4194304, (1, 33): 4194304, (33, 45): 4194304, (4, 33):
        4194304, (512, 115): 4194304, (4096, 115): 4194304},
    'rdrf_selftest_app_bwd_workspace_bytes': {(1, 1): 4194304, (1, 32): 4194304, (1, 33): 4194304, (33, 45): 4194304, (4, 33):
        4194304, (512, 115): 4194304, (4096, 115): 4194304},
    'rdrf_selftest_scatter_workspace_bytes': {(1, 1): 15616, (1, 32): 16896, (1, 33): 16896, (33, 45): 103936, (4, 33): 23296,
        (512, 115): 3719424, (4096, 115): 29686272},
    'rdrf_frame_depth_loss_workspace_bytes': {(1, 1): 264, (1, 32): 512, (1, 33): 520, (33, 45): 616, (4, 33): 520, (512, 115):
        1176, (4096, 115): 1176},
    'rdrf_flow_to_image_workspace_bytes': {(1, 1): 260, (1, 32): 260, (1, 33): 260, (33, 45): 280, (4, 33): 260, (512, 115): 1176,
        (4096, 115): 4352},
    'rdrf_compute_alpha_workspace_bytes': {(1, 1): 4195584, (1, 32): 4199424, (1, 33): 4199680, (33, 45): 4201216, (4, 33):
        4199680, (512, 115): 4210176, (4096, 115): 4210176},
    'rdrf_render_chunks_workspace_bytes': {(1, 1, 1): 8414208, (1, 1, 4): 33656832, (1, 32, 1): 8418304, (1, 32, 4): 33673216, (1,
        33, 1): 8418304, (1, 33, 4): 33673216, (33, 45, 1): 8615936, (33, 45, 4): 34463744, (4, 33, 1): 8432128, (4, 33, 4):
        33728512, (512, 115, 1): 16173056, (512, 115, 4): 64692224, (4096, 115, 1): 70488576, (4096, 115, 4): 281954304},
    'rdrf_ssim_workspace_bytes': {(1, 1, 1): 256, (1, 1, 3): 256, (1, 32, 1): 256, (1, 32, 3): 256, (1, 33, 1): 256, (1, 33, 3):
        256, (33, 45, 1): 288, (33, 45, 3): 352, (4, 33, 1): 256, (4, 33, 3): 256, (512, 115, 1): 1280, (512, 115, 3): 3328,
        (4096, 115, 1): 8448, (4096, 115, 3): 24832},
    'rdrf_saved_bytes[0]': {(1, 1): 71576, (1, 32): 72320, (1, 33): 141976, (33, 45): 3314360, (4, 33): 353632, (512, 115):
        129603328, (4096, 115): 1036814080},
    'rdrf_saved_bytes_ex[0,0]': {(1, 1): 71576, (1, 32): 72320, (1, 33): 141976, (33, 45): 3314360, (4, 33): 353632, (512, 115):
        129603328, (4096, 115): 1036814080},
    'rdrf_saved_bytes_ex[0,1]': {(1, 1): 1688, (1, 32): 2432, (1, 33): 2456, (33, 45): 41400, (4, 33): 5216, (512, 115): 1480192,
        (4096, 115): 11830784},
    'rdrf_saved_bytes[1]': {(1, 1): 157848, (1, 32): 158592, (1, 33): 314264, (33, 45): 8758200, (4, 33): 1005152, (512, 115):
        303208448, (4096, 115): 2425653248},
    'rdrf_saved_bytes_ex[1,0]': {(1, 1): 157848, (1, 32): 158592, (1, 33): 314264, (33, 45): 8758200, (4, 33): 1005152, (512,
        115): 303208448, (4096, 115): 2425653248},
    'rdrf_saved_bytes_ex[1,1]': {(1, 1): 75672, (1, 32): 76416, (1, 33): 150168, (33, 45): 4907704, (4, 33): 595296, (512, 115):
        152475392, (4096, 115): 1219790592},
    'rdrf_saved_bytes[2]': {(1, 1): 33024, (1, 32): 33024, (1, 33): 65792, (33, 45): 1540352, (4, 33): 164096, (512, 115):
        60293376, (4096, 115): 482345216},
    'rdrf_saved_bytes_ex[2,0]': {(1, 1): 33024, (1, 32): 33024, (1, 33): 65792, (33, 45): 1540352, (4, 33): 164096, (512, 115):
        60293376, (4096, 115): 482345216},
    'rdrf_saved_bytes_ex[2,1]': {(1, 1): 33024, (1, 32): 33024, (1, 33): 65792, (33, 45): 1540352, (4, 33): 164096, (512, 115):
        60293376, (4096, 115): 482345216},
    'rdrf_features_workspace_bytes': {1: 4442880, 32: 4442880, 33: 4638976, 77: 4835584, 4096: 29385472},
    'rdrf_features_bwd_workspace_bytes': {1: 4355360, 32: 4355360, 33: 4500032, 77: 4644704, 4096: 22728704},
    'rdrf_features_saved_bytes[0]': {1: 75904, 32: 75904, 33: 150272, 77: 224640, 4096: 9520640},
    'rdrf_features_saved_bytes[1]': {1: 162176, 32: 162176, 33: 322560, 77: 482944, 4096: 20530944},
}

KEPT = ["rdrf_forward_workspace_bytes", "rdrf_render_workspace_bytes", "rdrf_render_chunks_workspace_bytes",
        "rdrf_render_motion_workspace_bytes", "rdrf_flow_to_image_workspace_bytes", "rdrf_ssim_workspace_bytes",
        "rdrf_frame_depth_loss_workspace_bytes"] + [k for k in PARENT if "saved_bytes" in k]
DERIVED = ["rdrf_workspace_bytes", "rdrf_features_bwd_workspace_bytes", "rdrf_selftest_warp_bwd_workspace_bytes",
           "rdrf_selftest_heads_bwd_workspace_bytes", "rdrf_selftest_app_bwd_workspace_bytes",
           "rdrf_selftest_scatter_workspace_bytes", "rdrf_compute_alpha_workspace_bytes"]


def _call(key, shape):
    import ctypes as C
    L = pkg()
    name, _, fixed = key.partition("[")
    args = [int(v) for v in fixed.rstrip("]").split(",") if v] + list(shape if isinstance(shape, tuple) else (shape,))
    if name == "rdrf_saved_bytes_ex":      # (kind, N, S, flags): the flags come last
        args = [args[0], args[2], args[3], args[1]]
    fn = getattr(L.lib, name)
    fn.restype, fn.argtypes = C.c_size_t, [C.c_int] * len(args)
    return int(fn(*args))


def test_the_table_covers_every_exported_size_function_at_the_agreed_shapes():
    L = pkg()
    exported = {s for s in L.SYMBOLS if s.endswith("_workspace_bytes") or "_saved_bytes" in s}
    assert {k.partition("[")[0] for k in PARENT} == exported
    assert sorted(KEPT + DERIVED + ["rdrf_features_workspace_bytes"]) == sorted(PARENT)
    for key, row in PARENT.items():
        name = key.partition("[")[0]
        if "features" in name:
            assert list(row) == MS, key
        elif name == "rdrf_render_chunks_workspace_bytes":
            assert list(row) == [ns + (k,) for ns in NS for k in (1, 4)]
        elif name == "rdrf_ssim_workspace_bytes":
            assert list(row) == [ns + (c,) for ns in NS for c in (1, 3)]
        else:
            assert list(row) == NS, key


@pytest.mark.parametrize("key", KEPT)
def test_kept_sizes_return_the_parents_values(key):
    assert {shape: _call(key, shape) for shape in PARENT[key]} == PARENT[key]


def _non_decreasing(key):
    """in each argument with the others held: over the shapes of the table that differ in that argument alone, and over a walk
    through every value the table uses for it"""
    shapes = [s if isinstance(s, tuple) else (s,) for s in PARENT[key]]
    for i in range(len(shapes[0])):
        values = sorted({s[i] for s in shapes})
        for s in shapes:
            got = [_call(key, s[:i] + (v,) + s[i + 1:]) for v in values]
            assert got == sorted(got), (key, s, i, got)


@pytest.mark.parametrize("key", DERIVED)
def test_derived_sizes_never_exceed_the_parents(key):
    for shape, parent in PARENT[key].items():
        got = _call(key, shape)
        print(key, shape, "parent", parent, "now", got)
        assert 0 < got <= parent, (key, shape, got, parent)
        assert got % 256 == 0, (key, shape, got)
    _non_decreasing(key)


def test_features_workspace_keeps_its_form():
    key = "rdrf_features_workspace_bytes"
    for M, parent in PARENT[key].items():
        Np = (M + 31) // 32
        got = _call(key, M)
        assert got == _call("rdrf_workspace_bytes", (Np, 32)) + Np * 32 * (32 * 4 + 27 * 4 + 8) + (1 << 14)
        assert 0 < got <= parent, (M, got, parent)
    _non_decreasing(key)


@pytest.mark.parametrize("N,S", NS)
def test_training_workspace_covers_the_forward(N, S):
    assert _call("rdrf_workspace_bytes", (N, S)) >= _call("rdrf_forward_workspace_bytes", (N, S))
