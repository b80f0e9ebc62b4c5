"""``plan_voxel_gradient`` (csrc/drr_common.hiph): the one host-side decision on which kernels compute a voxel gradient, shown to the
host by ``xvr_drr_voxel_gradient_plan``.  No GPU: nothing is launched.

``tests/golden/grad_plan_rows.txt`` was recorded from the code before the planner existed (commit c659a52): a scratch patch of
``launch_gather`` and of the two ``xvr_drr_*_backward`` bodies wrote the fields below into a buffer just before their first HIP call
(``GatherArgs`` as filled, the arm of the launch chain as ``family``, the memsets, the scatter launches behind) and returned, driven
through ctypes with stand-in pointers over the cases of ``CASES`` -- the edges of every condition the dispatch had.  A row holds what
the parent had decided by the time it returned: an early return (an error, a later slab that does nothing) records fewer fields.
The planner must reproduce every recorded field of every row."""
import ast
import ctypes
from pathlib import Path

import pytest

from xvr_amd import _lib
from xvr_amd.renderers import make_cspec
from xvr_amd.spec import RenderSpec

# r: renderer t / s; H x W detector, gw: spec.ray_grid_w (None: W); map: Siddon index map (exact, norm_dims_offset +1 / -1, align_corners);
# C: 0 = no mask, else channels of a masked render; gs / ss / fast: options gather_splat / siddon_splat / siddon_gather_fast;
# ws: workspace = exactly xvr_drr_backward_workspace_bytes ("full"), a byte less ("short"), that plus the per-cell scratch ("cells"), a byte
# less ("cells_short"), NULL ("none"), or off a 16-byte boundary ("misaligned"); slab: (slab_index, slab_count)
DEFAULT = dict(r="t", shape=(9, 7, 11), B=2, H=6, W=5, gw=None, map="exact", C=0, clip=0, n_points=50, gs=1, ss=1, fast=1,
               ws="cells", slab=(0, 1), gpose=1, gvol=1)
MAPS = {"exact": {}, "+1": {"norm_dims_offset": 1}, "-1": {"norm_dims_offset": -1}, "ac": {"align_corners": True}}


def _rows():
    rows = []
    for line in (Path(__file__).parent / "golden" / "grad_plan_rows.txt").read_text().splitlines():
        if line.startswith("#"):
            continue
        case, fields, wants_cells = line.split(" | ")
        want = {k: tuple(map(int, v.split(","))) if "," in v else float(v) for k, v in (f.split("=") for f in fields.split())}
        rows.append((ast.literal_eval(case), want, int(wants_cells)))
    return rows


ROWS = _rows()


class GradPlan(ctypes.Structure):   # include/xvr_drr.h: xvr_drr_grad_plan
    _fields_ = [("cmax_offset", ctypes.c_int64), ("cells_offset", ctypes.c_int64)] + [
        (n, ctypes.c_int32 * 3 if n in ("bd", "olo") else ctypes.c_float if n == "spv_limit" else ctypes.c_int32) for n in (
            "error", "noop", "siddon", "gather", "family", "clip", "mask", "nx", "exact", "V", "bd", "cmax_stride", "cells_wanted", "cells", "olo",
            "only_if_fine", "spv_limit", "fine_pair", "bx0", "bxn", "later_slab", "zero_flag_line", "zero_brick_queue", "zero_cmax",
            "zero_xcd_queues", "tail_pose", "tail_volume", "tail_guarded", "tail_resident")]


def _plan(lib, case, ws=None):
    c = dict(DEFAULT, **case)
    siddon, n = c["r"] == "s", c["H"] * c["W"]
    spec = RenderSpec(renderer="siddon" if siddon else "trilinear", n_points=c["n_points"], clip_to_volume=bool(c["clip"]), **MAPS[c["map"]])
    cs = make_cspec(c["shape"], spec, ray_grid_w=c["W"] if c["gw"] is None else c["gw"])
    base = lib.xvr_drr_backward_workspace_bytes(c["B"], n, *c["shape"])
    cells = ((base + 255) & ~255) + 32 * c["shape"][0] * c["shape"][1] * c["shape"][2]
    ws = ws or c["ws"]
    nbytes = {"full": base, "short": base - 1, "cells": cells, "cells_short": cells - 1, "none": cells, "misaligned": cells}[ws]
    plan = GradPlan()
    with _lib.option("gather_splat", c["gs"]), _lib.option("siddon_splat", c["ss"]), _lib.option("siddon_gather_fast", c["fast"]):
        rc = lib.xvr_drr_voxel_gradient_plan(int(siddon), int(c["C"] > 0), *c["shape"], max(c["C"], 1), c["B"], n, ctypes.byref(cs), c["gvol"], c["gpose"],
                                             nbytes, int(ws not in ("none", "misaligned")), c["slab"][0], c["slab"][1], ctypes.byref(plan))
        sized = lib.xvr_drr_siddon_backward_workspace_bytes(c["B"], n, *c["shape"], ctypes.byref(cs)) if siddon else base
    assert rc == plan.error
    return plan, sized, base, cells


def test_rows_cover_the_edges_they_claim():
    cases = [dict(DEFAULT, **c) for c, _, _ in ROWS]
    assert len(ROWS) == 292 and {c["r"] for c in cases} == {"t", "s"} and {c["map"] for c in cases} == set(MAPS)
    families = {w.get("family") for _, w, _ in ROWS}
    assert families >= set(range(1, 10)), families        # every arm of the launch chain
    assert {w["error"] for _, w, _ in ROWS} == {0, -1}     # (no recorded case reaches "detector too small" or "grid too large": 4 n >= 4)


@pytest.mark.parametrize("i", range(len(ROWS)))
def test_planner_reproduces_the_recorded_row(i):
    lib = _lib.load()
    case, want, wants_cells = ROWS[i]
    plan, sized, base, cells = _plan(lib, case)
    got = {k: tuple(getattr(plan, k)) if k in ("bd", "olo") else getattr(plan, k) for k in want}
    assert got == want, (case, {k: (got[k], want[k]) for k in want if got[k] != want[k]})
    # the sizing function is the plan's answer: base plus the per-cell scratch exactly when the spec wants the cells, and a workspace of that
    # size is then what makes a usable, unmasked, volume-wanting call take them
    assert sized == (cells if wants_cells else base) and wants_cells == plan_wants(lib, case)
    if dict(DEFAULT, **case)["r"] == "s":
        roomy, _, _, _ = _plan(lib, dict(case, C=0, gvol=1, slab=(0, 1)), ws="cells")
        assert roomy.cells == (wants_cells and roomy.gather) and (roomy.cells_offset == ((base + 255) & ~255) if roomy.cells else roomy.cells_offset == -1)


def plan_wants(lib, case):
    return _plan(lib, dict(case, C=0, gvol=1, slab=(0, 1)), ws="none")[0].cells_wanted if dict(DEFAULT, **case)["r"] == "s" else 0


def test_plan_export_is_declared_bound_and_refuses_nulls():
    lib = _lib.load()
    assert "xvr_drr_voxel_gradient_plan" in (Path(__file__).parents[1] / "include" / "xvr_drr.h").read_text()
    assert "xvr_drr_voxel_gradient_plan" in _lib.EXPORTS and lib.xvr_drr_abi_version() == 12
    assert lib.xvr_drr_voxel_gradient_plan(0, 0, 9, 7, 11, 1, 1, 30, None, 1, 1, 0, 0, 0, 1, None) == -1
    assert b"null" in lib.xvr_drr_last_error()
