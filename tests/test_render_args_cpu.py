"""The evaluation render's argument checks without a GPU: every entry point of the family is called with arguments it refuses
before any launch, and the return code and the rdrf_last_error() text are held to what the library gave before the entry points
shared one call record and one set of checks (recorded from that build; a caller may match on these texts).

No case can reach a launch: the parameter structs hold no factor grids, so the last check of every path (the component
counts) refuses whatever the earlier ones let through; the one case with valid grids (the masked render's workspace check,
which comes after them) has a short workspace.  Pointers other than the structs are never read: they point at a dummy."""
import ctypes as C

import pytest

from _util import pkg

L = pkg()

NDC, CONTRACT, WORLD = 0, 1, 2
N0, S0 = 5, 7
STEP_RULE = ("render: ray_type ndc / contract through rdrf_render_*_fwd, any other through rdrf_render_world_fwd with step > 0 "
             "(ray_type %d, step %s)")

_dummy = (C.c_char * 256)()
PTR = C.addressof(_dummy)


def _grids(vm, c0, c1):
    for i in range(3):
        vm.C[i], vm.W[i], vm.H[i], vm.L[i] = (c0 if i == 0 else c1), 8, 8, 8


def _scene(ray_type=NDC, grids=False):
    PS, PD, cs, cd = L.RdrfStaticParams(), L.RdrfDynamicParams(), L.RdrfFieldCfg(), L.RdrfFieldCfg()
    PS.packed_fwd = PD.packed_fwd = PTR   # (the chunk loop asks for both before anything else)
    cs.ray_type = cd.ray_type = ray_type
    if grids:
        _grids(PS.density, 16, 4), _grids(PS.app, 48, 12), _grids(PD.density, 16, 4), _grids(PD.blending, 16, 4), _grids(PD.app, 48, 12)
    return PS, cs, PD, cd


def _call(entry, N=N0, S=S0, ray_type=NDC, null_ps=False, step=None, short_ws=False, chunk=4, grids=False, mask=True,
          cams=True, seeds=True, ws_bytes=None):
    """the entry point on a refusable call; returns (rc, last error text)"""
    PS, cs, PD, cd = _scene(ray_type, grids)
    keep = [PS, cs, PD, cd]
    head = (None if null_ps else C.byref(PS), C.byref(cs), C.byref(PD), C.byref(cd), PTR, PTR, N, S)
    maps = L.RenderMapsC()
    size = {"rdrf_render_chunks_fwd": lambda: L.lib.rdrf_render_chunks_workspace_bytes(min(chunk, N), S, 1),
            "rdrf_render_chunks_maps_fwd": lambda: L.lib.rdrf_render_chunks_workspace_bytes(min(chunk, N), S, 1),
            "rdrf_render_masked_fwd": lambda: L.lib.rdrf_render_masked_ws_bytes(N, S)}.get(
                entry, lambda: L.lib.rdrf_render_workspace_bytes(N, S))
    if ws_bytes is None:
        ws_bytes = size() - (1 if short_ws else 0)
    near, far, fn = 0.0, 1.0, getattr(L.lib, entry)
    if entry in ("rdrf_render_fwd", "rdrf_render_sequence_fwd", "rdrf_render_fused_fwd"):
        rc = fn(*head, near, far, PTR, PTR, PTR, ws_bytes, None)
    elif entry == "rdrf_render_maps_fwd":
        rc = fn(*head, near, far, 0, C.byref(maps), PTR, ws_bytes, None)
    elif entry == "rdrf_render_chunks_fwd":
        rc = fn(*head, chunk, near, far, PTR, PTR, PTR, ws_bytes, None, None, 0)
    elif entry == "rdrf_render_chunks_maps_fwd":
        rc = fn(*head, chunk, near, far, C.byref(maps), PTR, ws_bytes, None, None, 0)
    elif entry == "rdrf_render_world_fwd":
        rc = fn(*head, 0, near, far, 0.25 if step is None else step, 0, C.byref(maps), PTR, ws_bytes, None, None, 0)
    elif entry == "rdrf_render_masked_fwd":
        m = L.RdrfAlphaMask()
        m.bits, m.T = PTR, 1
        m.grid[0] = m.grid[1] = m.grid[2] = 4
        keep.append(m)
        rc = fn(*head, near, far, 0.0 if step is None else step, C.byref(m) if mask else None, None, C.byref(maps), None, PTR,
                ws_bytes, None)
    elif entry == "rdrf_render_motion_fwd":
        cam, mm = L.MotionCamsC(4, 4, PTR, PTR, PTR, 0), L.MotionMapsC()
        rc = fn(*head, near, far, 0, C.byref(maps), C.byref(cam) if cams else None, C.byref(mm), PTR, ws_bytes, None)
    elif entry == "rdrf_render_track_seeds_fwd":
        rc = fn(*head, near, far, C.byref(maps), PTR if seeds else None, PTR, ws_bytes, None)
    else:
        raise KeyError(entry)
    del keep
    return rc, L.lib.rdrf_last_error().decode()


ENTRIES = ("rdrf_render_fwd", "rdrf_render_sequence_fwd", "rdrf_render_fused_fwd", "rdrf_render_maps_fwd", "rdrf_render_chunks_fwd",
           "rdrf_render_chunks_maps_fwd", "rdrf_render_world_fwd", "rdrf_render_masked_fwd", "rdrf_render_motion_fwd",
           "rdrf_render_track_seeds_fwd")
NATIVE_RAYS = {"rdrf_render_world_fwd": WORLD}   # the ray type an entry point is called with where the case sets none

BAD = "render: bad arguments"
SMALL = "render: workspace too small"
# (return code, rdrf_last_error()) per case and entry point, as the library before this refactor gave them
EXPECT = {
    "null_PS": {
        "rdrf_render_fwd": (-1, BAD), "rdrf_render_sequence_fwd": (-1, BAD), "rdrf_render_fused_fwd": (-1, BAD),
        "rdrf_render_maps_fwd": (-1, BAD), "rdrf_render_chunks_fwd": (-1, "render_chunks: bad arguments"),
        "rdrf_render_chunks_maps_fwd": (-1, "render_chunks: bad arguments"), "rdrf_render_world_fwd": (-1, BAD),
        "rdrf_render_masked_fwd": (-1, "render_masked: bad arguments"), "rdrf_render_motion_fwd": (-1, BAD),
        "rdrf_render_track_seeds_fwd": (-1, BAD)},
    "S_0": {
        "rdrf_render_fwd": (-1, BAD), "rdrf_render_sequence_fwd": (-1, BAD), "rdrf_render_fused_fwd": (-1, BAD),
        "rdrf_render_maps_fwd": (-1, BAD), "rdrf_render_chunks_fwd": (-1, "render_chunks: bad arguments"),
        "rdrf_render_chunks_maps_fwd": (-1, "render_chunks: bad arguments"), "rdrf_render_world_fwd": (-1, BAD),
        "rdrf_render_masked_fwd": (-1, "render_masked: bad arguments"), "rdrf_render_motion_fwd": (-1, BAD),
        "rdrf_render_track_seeds_fwd": (-1, BAD)},
    "short_ws": {
        "rdrf_render_fwd": (-3, SMALL), "rdrf_render_sequence_fwd": (-3, SMALL), "rdrf_render_fused_fwd": (-3, SMALL),
        "rdrf_render_maps_fwd": (-3, SMALL), "rdrf_render_chunks_fwd": None, "rdrf_render_chunks_maps_fwd": None,
        "rdrf_render_world_fwd": (-3, SMALL), "rdrf_render_masked_fwd": None, "rdrf_render_motion_fwd": (-3, SMALL),
        "rdrf_render_track_seeds_fwd": (-3, SMALL)},
}


@pytest.mark.parametrize("entry", ENTRIES)
def test_empty_batch_is_a_no_op(entry):
    rc, _ = _call(entry, N=0, null_ps=True, ray_type=NATIVE_RAYS.get(entry, NDC))
    assert rc == 0


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("case", ["null_PS", "S_0", "short_ws"])
def test_shared_prefix_is_refused(case, entry):
    kw = {"null_PS": dict(null_ps=True, N=1), "S_0": dict(S=0), "short_ws": dict(short_ws=True, grids=entry == "rdrf_render_masked_fwd")}[case]
    want = EXPECT[case][entry]
    if want is None:   # the texts that carry the sizes
        need = {"rdrf_render_masked_fwd": lambda: L.lib.rdrf_render_masked_ws_bytes(N0, S0)}.get(
            entry, lambda: L.lib.rdrf_render_chunks_workspace_bytes(4, S0, 1))()
        who = "render_masked" if entry == "rdrf_render_masked_fwd" else "render_chunks"
        want = (-3, f"{who}: workspace too small: need {need} have {need - 1}")
    assert _call(entry, ray_type=NATIVE_RAYS.get(entry, NDC), **kw) == want


@pytest.mark.parametrize("entry", ["rdrf_render_world_fwd", "rdrf_render_masked_fwd"])
def test_step_on_an_ndc_cfg(entry):
    want = {"rdrf_render_world_fwd": (-1, STEP_RULE % (NDC, "0.25")),
            "rdrf_render_masked_fwd": (-1, "render_masked: step > 0 exactly for the world-space march (ray_type 0, step 0.25)")}[entry]
    assert _call(entry, ray_type=NDC, step=0.25) == want


@pytest.mark.parametrize("entry", [e for e in ENTRIES if e != "rdrf_render_world_fwd"])
def test_world_cfg_through_another_entry_point(entry):
    want = {"rdrf_render_masked_fwd": (-1, "render_masked: step > 0 exactly for the world-space march (ray_type 2, step 0)"),
            "rdrf_render_motion_fwd": (-1, "render_motion: ray_type must be ndc or contract (renderer.py:1335-1351)"),
            "rdrf_render_track_seeds_fwd": (-1, "render_track_seeds: ray_type must be ndc or contract (renderer.py:1335-1351)")}.get(
                entry, (-1, STEP_RULE % (WORLD, "0")))
    assert _call(entry, ray_type=WORLD) == want


def test_unit_specific_refusals():
    assert _call("rdrf_render_world_fwd", ray_type=WORLD, step=0.0) == (-1, "render_world: step must be positive (the field's stepSize)")
    assert _call("rdrf_render_masked_fwd", mask=False) == (-1, "render_masked: at least one of the two masks must be given")
    assert _call("rdrf_render_motion_fwd", cams=False) == (-1, "render_motion: cameras and motion maps are required")
    assert _call("rdrf_render_track_seeds_fwd", seeds=False) == (-1, "render_track_seeds: no seed buffer")


def test_no_grids_is_the_last_refusal():
    """what every other case of this file relies on: with all else in order, parameter structs without factor grids are refused"""
    for entry in ENTRIES:
        who = "render_masked" if entry == "rdrf_render_masked_fwd" else "render"
        assert _call(entry, ray_type=NATIVE_RAYS.get(entry, NDC)) == (
            -1, f"{who}: only density comps {{16,4,4}} / app comps {{48,12,12}} of one grid are built"), entry


def test_chunk_coalescing_bound_is_formed_without_overflow():
    """chunk = 2^30 on 2^30 + 1 rays, one sample each, a workspace for one chunk: (g + 1) * chunk of the coalescing loop is 2^31.
    The loop must stop at its 32-bit sample-index guard, and the first chunk is then refused by the same bound of the render."""
    chunk = 1 << 30
    ws_bytes = L.lib.rdrf_render_chunks_workspace_bytes(chunk, 1, 0)
    assert _call("rdrf_render_chunks_fwd", N=chunk + 1, S=1, chunk=chunk, ws_bytes=ws_bytes) == (
        -1, "render: N * S * 3 must stay below 2^31: render in chunks")
