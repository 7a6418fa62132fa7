"""Which levels take the tail launch of the condensed apply (cond_tail_kernel: the Schur solve and the back substitution of a
patch in one workgroup): the rule of csrc/cond_layout.h (cond_tail) against its long-hand statement, and the maxima it reads on
a host plan.  CPU only."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "alfi_amd", "csrc")


@pytest.mark.parametrize("flags", [(), ("-DALFI_COND_TAIL=0",)], ids=["library", "ab-build"])
def test_truth_table_of_the_rule(tmp_path, flags):
    """tests/cond_tail_rule_check.cpp: max_xpairs 64 / 65, max_sc 32 / 33, max_s 64 / 65 among others; with ALFI_COND_TAIL=0
    (scripts/build_variant.sh) no level takes the launch"""
    exe = str(tmp_path / "cond_tail_rule_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-I", CSRC, *flags,
                           os.path.join(ROOT, "tests", "cond_tail_rule_check.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.startswith("OK "), r.stdout


def test_the_gpu_test_restates_the_same_rule():
    """tests/test_gpu_cond_tail.py decides on a host plan which form a level takes"""
    from tests.test_gpu_cond_tail import takes_tail
    for xp in (64, 65):
        for sc in (32, 33):
            for s in (64, 65):
                plan = {"xp_ptr": np.array([0, 3, 3 + xp]), "g_sc": np.array([1, sc]), "max_s": s}
                assert takes_tail(plan) == (xp <= 64 and sc <= 32 and s <= 64), (xp, sc, s)


def test_the_maxima_of_a_host_plan():
    """what tests/test_gpu_cond_tail.py reads from the tables of plan_condensed (CondPlan::max_xpairs, max_sc in csrc/patch_plan.h
    are the same maxima, taken where the tables are built)"""
    from alfi_amd import _hostlib
    from tests.test_gpu_cond_ahead import _shape, arrowhead_level
    from tests.test_gpu_cond_tail import maxima, takes_tail
    shapes = [_shape([7, 8, 1], [7, 8, 9], 9), _shape([], [], 4), _shape([8] * 9, [16] * 9, 17)]
    A, pp, pd, groups = arrowhead_level(2, shapes, 6, 0)
    plan = _hostlib.plan_condensed(2, A.rowptr, A.colidx, pp, pd, groups)
    assert maxima(plan) == (72, 32, 34) and plan["max_pairs"] == 9 * 16 and not takes_tail(plan)
    A, pp, pd, groups = arrowhead_level(2, shapes[:2], 6, 0)
    plan = _hostlib.plan_condensed(2, A.rowptr, A.colidx, pp, pd, groups)
    assert maxima(plan) == (16, 18, 18) and takes_tail(plan)
