"""The three levels the patch planners (csrc/patch_plan.h) are pinned on, shared by tests/test_patch_plan.py (CPU) and
tests/test_gpu_star_condense.py:

  a  2-D Scott-Vogelius [P2]^2, TwoDimLidDrivenCavityProblem(2), one refinement, the hierarchy's own patch_groups:
     25 macro stars of up to 62 dofs;
  b  3-D [P2+FB]^3, ThreeDimLidDrivenCavityProblem(2), one refinement, labels from find_groups: 125 vertex stars of up to 153
     dofs, 81 of them grouped;
  c  3-D Scott-Vogelius [P3]^3, ThreeDimLidDrivenCavityProblem(1), one refinement, patch_groups: 27 macro stars of up to 1599
     dofs -- more than 256 row pairs per patch (several CondChunks and sigma chunks each), workgroup-per-patch sweeps.

The sweeps use the two sort orders of tests/gpu_mult_schedule_worker.py, symmetrised."""
import functools

import numpy as np

SORT_ORDER = {"a": "0+:1-|1+:0-", "b": "0+:1-:2+", "c": "0+:1-:2+"}


@functools.lru_cache(maxsize=None)
def case(name):
    """(host level, group labels int32, iteration set int64)"""
    from alfi_amd import _hostlib
    from alfi_amd.problem import ThreeDimLidDrivenCavityProblem, TwoDimLidDrivenCavityProblem, build_hierarchy
    from alfi_amd.relaxation import Options, OrderedRelaxation
    from alfi_amd.sv import build_sv_hierarchy
    if name == "a":
        lv, _ = build_sv_hierarchy(TwoDimLidDrivenCavityProblem(2), 1, 2, Re=10.0)
    elif name == "b":
        lv, _ = build_hierarchy(ThreeDimLidDrivenCavityProblem(2), 1, 2, Re=1000.0)
    else:
        lv, _ = build_sv_hierarchy(ThreeDimLidDrivenCavityProblem(1), 1, 3, Re=100.0)
    L = lv[-1]
    if name == "b":
        groups = _hostlib.find_groups(L.bs, L.A.rowptr, L.A.colidx, L.patch_ptr, L.patch_dofs)
    else:
        groups = np.asarray(L.patch_groups, dtype=np.int32)
    orl = OrderedRelaxation()
    orl.name = "Star"
    orl.opts = Options("", {"pc_patch_construction_Star_sort_order": SORT_ORDER[name]})
    iterset = np.asarray(orl.iteration_order(L.V.mesh.coords[L.patch_seeds]), dtype=np.int64)
    return L, groups, iterset


@functools.lru_cache(maxsize=None)
def plans(name):
    """The host planners on the case: {"layout": ..., "cond": ..., "sweep": ...}, each a dict of tables and scalars."""
    from alfi_amd import _hostlib
    L, groups, iterset = case(name)
    return {"layout": _hostlib.plan_patch_layout(L.n, L.patch_ptr, L.patch_dofs),
            "cond": _hostlib.plan_condensed(L.bs, L.A.rowptr, L.A.colidx, L.patch_ptr, L.patch_dofs, groups),
            "sweep": _hostlib.plan_sweep(L.bs, L.A.rowptr, L.A.colidx, L.patch_ptr, L.patch_dofs, iterset, True)}
