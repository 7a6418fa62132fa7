"""CPU checks of block right-hand sides on levels of dense macro-star inverses: the width rule (csrc/block_cols.h:
block_big_lds, block_big_width), the work split the single and the block launcher share (csrc/patch_plan.h: big_split) and the
cutting of a chunk into pieces under host sanitizers -- a stand-alone program with its own main, as
tests/test_block_rhs_condensed.py builds its own --, the rule restated in Python on the levels that
tests/test_gpu_block_rhs_macro.py runs, and that the dispatch reads the named threshold and the shared work split."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "alfi_amd", "csrc")


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_width_rule_split_and_pieces_under_host_sanitizers(tmp_path):
    """tests/block_big_width_check.cpp: widths at max_np 160, 161, 2048, 2049, 2730, 2731, 4096; budgets of 0, exactly NV x lds,
    one byte less; big_split of the table's levels; ncol 1 .. 9 in pieces of every width"""
    exe = str(tmp_path / "block_big_width_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-I", CSRC,
                           os.path.join(ROOT, "tests", "block_big_width_check.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.startswith("OK "), r.stdout


def test_threshold_is_named_once_and_read_by_the_dispatch():
    sources = {f: _read(f) for f in os.listdir(CSRC) if f.endswith((".h", ".hip", ".cpp"))}
    defs = [f for f, s in sources.items() if re.search(r"constexpr\s+\w+\s+BIG_BLOCK_MIN_PATCHES\s*=", s)]
    assert defs == ["block_cols.h"]
    assert re.search(r"constexpr int64_t BIG_BLOCK_MIN_PATCHES = 8;", sources["block_cols.h"])
    assert "L->npatch < BIG_BLOCK_MIN_PATCHES" in sources["api_block.hip"]
    assert "block_big_width(L->lay.max_np, L->ctx->block_lds_bytes)" in sources["api_block.hip"]
    # no other literal 8-patch threshold next to it
    assert not re.search(r"npatch\s*<\s*8\b", sources["api_block.hip"])


def test_both_launchers_read_one_big_split():
    """big_split is defined once, in the host-only header, and both launchers call it"""
    sources = {f: _read(f) for f in os.listdir(CSRC) if f.endswith((".h", ".hip", ".cpp"))}
    defs = [f for f, s in sources.items() if re.search(r"\bint big_split\(int64_t npatch, int max_np\)\s*\{", s)]
    assert defs == ["patch_plan.h"]
    assert "big_split(p1 - p0, max_np)" in sources["kernels_bigpatch.hip"]
    assert "big_split(L->npatch, L->lay.max_np)" in sources["kernels_block_big.hip"]
    # the new kernel's LDS is the width rule's, not a static array of the largest patch there can be
    assert "block_big_lds(L->lay.max_np, NV)" in sources["kernels_block_big.hip"]
    assert "BIG_MAX_NP" not in sources["kernels_block_big.hip"] and "extern __shared__" in sources["kernels_block_big.hip"]


def test_the_python_restatement_and_the_levels_of_the_gpu_test():
    from tests import block_big_cases as bc
    assert [bc.block_big_width(m) for m in (160, 161, 2048, 2049, 2730, 2731, 4096)] == [4, 4, 4, 3, 3, 2, 2]
    assert bc.block_big_width(2175) == 3 and bc.block_big_width(2175, 69632) == 4 and bc.block_big_width(2175, 69631) == 3
    one = bc.block_big_lds(512, 1)
    assert [bc.block_big_width(512, b) for b in (3 * one, 2 * one, 2 * one - 1, 0)] == [3, 2, 0, 0]
    assert [bc.big_split(*a) for a in ((12, 2048), (27, 1599), (303, 1941), (1765, 2175), (5000, 4096))] == [4, 4, 4, 2, 1]
    for name, sizes in bc.LEVELS.items():
        assert 8 <= len(sizes) <= 16 and max(sizes) > 160 and len(set(sizes)) == len(sizes), name
        assert sum(8 * n * ((n + 1) & ~1) for n in sizes) < 0.1e9, name          # well under 0.3 GB of inverses
        assert (bc.big_split(len(sizes), max(sizes)), bc.block_big_width(max(sizes))) == bc.EXPECTED[name], name
    assert {n % 4 for n in bc.LEVELS["D"]} == {0, 1, 2, 3} and max(bc.SMALL_STARS) <= 64 < 2 * min(bc.SMALL_STARS)
    ptr, dofs = bc.patch_arrays((5, 3))
    assert ptr.tolist() == [0, 5, 8] and len(dofs) == 8 and all(dofs[i] < dofs[i + 1] for i in range(4)) and dofs.max() < bc.NDOF
