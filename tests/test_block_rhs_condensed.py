"""CPU checks of block right-hand sides on condensed levels: the width rule and the cutting of a chunk into pieces
(csrc/block_cols.h: block_cond_width, block_pieces, block_piece) under host sanitizers -- a stand-alone program with its own main,
as tests/test_block_rhs.py builds block_cols_check.cpp --, the rule restated in Python on the host plans of the levels that
tests/test_gpu_block_rhs_condensed.py runs, and that header, exports and ctypes table name the two new entry points."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = {"alfi_patch_apply_block_width": "alfi_level* lvl, int* width", "alfi_ctx_set_block_lds_bytes": "alfi_ctx* ctx, int64_t bytes"}


def test_width_rule_and_pieces_under_host_sanitizers(tmp_path):
    """tests/block_cond_width_check.cpp: budgets of 0, exactly NV x lds, one byte less; ncol 1 .. 9 in pieces of every width"""
    exe = str(tmp_path / "block_cond_width_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "alfi_amd", "csrc"),
                           os.path.join(ROOT, "tests", "block_cond_width_check.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.startswith("OK "), r.stdout


def test_new_entry_points_are_declared_exported_and_bound():
    from alfi_amd import _lib
    header = open(os.path.join(ROOT, "include", "alfi_hip.h")).read()
    lib = _lib.load()
    for name, args in NEW_SYMBOLS.items():
        assert "int %s(%s);" % (name, args) in header, name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    from alfi_amd import hip
    assert callable(hip.Level.patch_apply_block_width) and callable(hip.Context.set_block_lds_bytes)
    # the threshold is named once and both launchers read it
    csrc = os.path.join(ROOT, "alfi_amd", "csrc")
    assert "COND_PER_PATCH_MIN = 1024" in open(os.path.join(csrc, "cond_layout.h")).read()
    assert "p1 - p0 < COND_PER_PATCH_MIN" in open(os.path.join(csrc, "kernels_bigpatch.hip")).read()
    assert "L->npatch < COND_PER_PATCH_MIN" in open(os.path.join(csrc, "api_block.hip")).read()


def test_expected_widths_of_the_vertex_star_plan():
    """The [P2+FB]^3 vertex stars (tests/patch_plan_cases.py, case b: full stars of 153 dofs, 6 groups of 15, a skeleton of 63):
    the one-vector front launch asks for (153 + 90 + 6 x 27 + 2) x 8 bytes, the back launch for less, and four columns fit the
    default budget many times over."""
    from tests.block_cond_cases import expected_width
    from tests.patch_plan_cases import plans
    pl = plans("b")["cond"]
    assert pl["lds_front"] == (153 + 90 + 6 * 27 + 2) * 8 and pl["lds_back"] == (63 + 6 * 27 + 2) * 8
    per = max(pl["lds_front"], pl["lds_back"])
    assert expected_width(pl) == 4
    assert [expected_width(pl, k * per) for k in (4, 3, 2, 1, 0)] == [4, 3, 2, 0, 0]
    assert [expected_width(pl, k * per - 1) for k in (4, 3, 2)] == [3, 2, 0]
    assert pl["max_pairs"] == 6 * 14                         # row pairs of B: two waves per patch


def test_repeating_a_patch_set_repeats_its_groups():
    from tests.block_cond_cases import repeat_patches
    pp = np.array([0, 2, 5], dtype=np.int64)
    pd = np.array([4, 9, 1, 2, 3], dtype=np.int32)
    g = np.array([0, -1, 1, 1, -1], dtype=np.int32)
    p3, d3, g3 = repeat_patches(pp, pd, g, 5)
    assert p3.tolist() == [0, 2, 5, 7, 10, 12] and p3.dtype == np.int64
    assert d3.tolist() == [4, 9, 1, 2, 3, 4, 9, 1, 2, 3, 4, 9] and g3.tolist() == [0, -1, 1, 1, -1, 0, -1, 1, 1, -1, 0, -1]
    p1, d1, g1 = repeat_patches(pp, pd, None, 2)
    assert p1.tolist() == [0, 2, 5] and g1 is None and d1.tolist() == pd.tolist()
