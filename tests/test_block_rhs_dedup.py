"""CPU checks of block right-hand sides in the de-duplicated level product: the width rule (csrc/block_cols.h: block_dedup_lds,
block_dedup_width) and the cutting of a chunk into pieces under host sanitizers -- a stand-alone program with its own main, as
tests/test_block_rhs_macro.py builds its own --, the rule restated in Python on the operators that
tests/test_gpu_block_rhs_dedup.py runs (their block counts, tails and distinct columns per group counted with NumPy, so that the
widths the GPU test expects are derived, not copied from the library), and that header, exports and ctypes table name the new
entry point."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "alfi_amd", "csrc")


def test_width_rule_and_pieces_under_host_sanitizers(tmp_path):
    """tests/block_dedup_width_check.cpp: widths at 1, 682, 683, 910, 911, 1024 distinct columns for bs 2 and 3; budgets of 0,
    exactly NV x lds, one byte less; ncol 1 .. 9 in pieces of every width"""
    exe = str(tmp_path / "block_dedup_width_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-I", CSRC,
                           os.path.join(ROOT, "tests", "block_dedup_width_check.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.startswith("OK "), r.stdout


def test_the_python_restatement_of_the_width_rule():
    from tests import block_dedup_cases as dc
    sizes = (1, 682, 683, 910, 911, 1024)
    assert [dc.block_dedup_width(m, 2) for m in sizes] == [4, 4, 4, 4, 4, 4]
    assert [dc.block_dedup_width(m, 3) for m in sizes] == [4, 4, 3, 3, 2, 2]
    for bs in (2, 3):
        for m in sizes:
            one = dc.block_dedup_lds(m, bs, 1)
            assert one == 8 * bs * m
            assert [dc.block_dedup_width(m, bs, b) for b in (0, one, 2 * one - 1, 2 * one, 3 * one - 1, 3 * one, 4 * one - 1, 4 * one,
                                                             100 * one)] == [0, 0, 0, 2, 2, 3, 3, 4, 4]
    assert dc.block_dedup_width(0, 3) == 0
    # the budgets of the GPU test on pattern("ragged") at bs 3 (1024 distinct columns in one group)
    assert dc.block_dedup_lds(1024, 3, 2) == 2 * 24 * 1024 == 49152 and dc.block_dedup_lds(1024, 3, 4) == 98304
    assert [dc.block_dedup_width(1024, 3, b) for b in (49152, 49151, 98304, 98303)] == [2, 0, 4, 3]


def test_the_operators_of_the_gpu_test():
    """block counts, tails, idle waves of the last workgroup, distinct columns per group, default widths"""
    from tests import block_dedup_cases as dc
    want = {("long", 400): (400, 1597, 573, 1, [400, None], (4, 4)),
            ("long", 800): (800, 3197, 125, 3, [800, None, None, None], (4, 3)),
            ("pattern", "ragged"): (1200, 3379, 307, 2, [744, 1024, 136, 1], (4, 2)),
            ("pattern", "exact"): (1917, 4096, 0, 0, [822, 1024, 137, 1], (4, 2))}
    assert set(want) == set(dc.CASES)
    for (kind, arg), (nb, nnzb, tail, idle, distinct, widths) in want.items():
        n, rowptr, colidx = dc.structure(kind, arg)
        assert n == nb == len(rowptr) - 1 and rowptr[-1] == nnzb == len(colidx) and nnzb % dc.SPMV_WG == tail
        nchunks = -(-nnzb // dc.SPMV_CHUNK)
        assert (-nchunks) % 4 == idle                                  # waves of the last workgroup whose chunk is past nchunks
        assert dc.dedups(rowptr) and colidx.min() >= 0 and colidx.max() < nb
        for i in range(nb):                                            # sorted, distinct columns in every row
            assert np.all(np.diff(colidx[rowptr[i]:rowptr[i + 1]]) > 0)
        got = dc.group_distinct(colidx)
        assert len(got) == len(distinct) and all(d is None or d == g for d, g in zip(distinct, got)), got
        assert max(got) == max(d for d in distinct if d)
        assert (dc.expected_width(kind, arg, 2), dc.expected_width(kind, arg, 3)) == widths
        A = dc.operator(kind, arg, 3)
        assert A.nnzb == nnzb and A.vals.shape == (nnzb, 3, 3)
    # long: the whole of row 0 lies in group 0 and is longer than a chunk
    for nb in (400, 800):
        _, rowptr, _ = dc.structure("long", nb)
        assert dc.SPMV_CHUNK < rowptr[1] == nb <= dc.SPMV_WG and np.all(np.diff(rowptr)[1:] == 3)
    # pattern: the row starts the kernel's scan has to meet
    _, rowptr, colidx = dc.structure("pattern", "ragged")
    starts = rowptr[:9].tolist()
    assert starts == [0, 320, 384, 512, 768, 1023, 1024, 2124, 2187]
    assert 320 % 256 == 64 and 320 % 64 == 0                           # lane 0 of a later wave iteration
    assert 1023 % 64 == 63                                             # a row start at lane 63
    assert 1024 // dc.SPMV_WG != (2124 - 1) // dc.SPMV_WG and (2124 - 1) // 256 - 1024 // 256 + 1 == 5   # a group boundary, five chunks
    assert np.all(np.diff(rowptr)[8:] == 1) and np.all(colidx[2187:] == 0)
    assert not dc.dedups(np.array([0, 300, 600, 900]))                  # under 1024 blocks: the flat product


def test_new_entry_point_is_declared_exported_and_bound():
    from alfi_amd import _lib, hip
    header = open(os.path.join(ROOT, "include", "alfi_hip.h")).read()
    lib = _lib.load()
    name = "alfi_spmv_block_width"
    assert "int %s(alfi_level* lvl, int* width);" % name in header
    assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.SIGNATURES[name] == _lib.SIGNATURES["alfi_patch_apply_block_width"]
    assert callable(hip.Level.spmv_block_width)
    # the kernel's LDS is the width rule's, not a static array of the most columns a group can have
    kernel, dispatch = (open(os.path.join(CSRC, f)).read() for f in ("kernels_block_dedup.hip", "kernels_block.hip"))
    assert "block_dedup_lds(A.max_uniq, BS, NV)" in kernel and "extern __shared__" in kernel and "SPMV_DEDUP_MAX * BS" not in kernel
    assert "block_dedup_width(A.max_uniq, A.bs, budget_bytes)" in dispatch
