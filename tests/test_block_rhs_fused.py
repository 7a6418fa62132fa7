"""CPU checks of the block form of the four-launch smoother iteration: the dispatch rule and the partial-buffer sizing of
csrc/block_cols.h under host sanitizers (a stand-alone program with its own main, as tests/test_block_rhs_macro.py builds its
own), the rule restated in Python (tests/block_fused_cases.py) on the levels that tests/test_gpu_block_rhs_fused.py runs, and that
header, exports and ctypes table name the two new entry points."""
import itertools
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "alfi_amd", "csrc")

NEW_SYMBOLS = ["alfi_smooth_fgmres_block_mode", "alfi_ctx_set_block_fused"]


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_dispatch_rule_and_partial_sizing_under_host_sanitizers(tmp_path):
    """tests/block_smooth_mode_check.cpp: every combination of the rule's facts, the named cases, a buffer of every slot count
    written at its last entries, the rounding of the dot vectors, the pieces of a chunk of slots"""
    exe = str(tmp_path / "block_smooth_mode_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-I", CSRC,
                           os.path.join(ROOT, "tests", "block_smooth_mode_check.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.startswith("OK "), r.stdout


def test_new_entry_points_are_declared_exported_and_bound():
    from alfi_amd import _lib, hip
    header = open(os.path.join(ROOT, "include", "alfi_hip.h")).read()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert "int %s(" % name in header, name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert hasattr(hip.Level, "smooth_block_mode") and hasattr(hip.Context, "set_block_fused")
    # the old query keeps its meaning, and the header says so
    assert "alfi_smooth_fgmres_block_info keeps its meaning" in header


def test_the_python_restatement_is_the_header_rule():
    """the restatement agrees with the text of block_cols.h (the program above checks the compiled rule against the same long
    form), and the dispatch reads the rule from the header"""
    from tests import block_fused_cases as fc
    src = _read("block_cols.h")
    body = re.search(r"inline int block_smooth_mode\(const BlockSmoothFacts& f\) \{(.*?)\n\}", src, re.S).group(1)
    assert [ln.strip() for ln in body.strip().split("\n")] == [
        "if (!f.block_kernels || f.partitioned) return BLOCK_SMOOTH_LOOP;",
        "if (!f.fused_iteration) return BLOCK_SMOOTH_LOCKSTEP;",
        "if (!f.block_fused) return BLOCK_SMOOTH_LOOP;",
        "return f.applies_il || f.apply_waves != 0 || f.piece_width >= 2 ? BLOCK_SMOOTH_FUSED : BLOCK_SMOOTH_LOOP;"]
    for kern, fused, part, fi, il in itertools.product((False, True), repeat=5):
        for waves, width in itertools.product((0, 1, 4, 8), (0, 1, 2, 3, 4)):
            want = 0 if (not kern or part) else 1 if not fi else 0 if not fused else 2 if (il or waves or width >= 2) else 0
            assert fc.block_smooth_mode(kern, fused, part, fi, il, waves, width) == want
    assert fc.block_partial_per_slot() == 2 * 1024 * 32
    assert re.search(r"constexpr int RED_BLOCKS = 1024;", _read("common.h")) and re.search(r"constexpr int RED_MAXV = 32;", _read("common.h"))
    assert [fc.block_dot_vectors(v) for v in (0, 1, 4, 5, 8, 9, 16, 17)] == [0, 4, 4, 8, 8, 16, 16, 0]
    api = _read("api_block.hip")
    assert "return block_smooth_mode(f);" in api and "block_partial_per_slot(RED_BLOCKS, RED_MAXV)" in api
    assert len(re.findall(r"\bblock_smooth_mode\(const BlockSmoothFacts", "".join(_read(f) for f in os.listdir(CSRC)
                                                                                 if f.endswith((".h", ".hip", ".cpp"))))) == 1


def test_the_levels_of_the_gpu_test_take_the_paths_it_means():
    from tests import block_fused_cases as fc
    lanes = set()
    for (bs, half), lpr in fc.BANDS.items():
        A = fc.banded_operator(fc.NB, half, bs, 1)
        assert fc.spmv_dot_lanes(bs, A.nnzb, fc.NB) == lpr and fc.NB % (256 // lpr) != 0
        assert fc.takes_fused_iteration(bs * fc.NB, 2 * half + 1, 15) and not fc.takes_fused_iteration(bs * fc.NB, 2 * half + 1, 16)
        lanes.add((bs, lpr))
    assert lanes == {(2, 4), (2, 8), (2, 32), (3, 8), (3, 16), (3, 32)}
    assert (3 * fc.NB) % 2 == 1                                   # bs 3: an odd vector length
    # the grid-stride level: two passes of the product's loop, more dot partials than one pass of the consumer's sum takes
    rows_per_pass = fc.RED_BLOCKS * (256 // 4)
    assert rows_per_pass < fc.NB_STRIDE <= 2 * rows_per_pass and fc.RED_BLOCKS > 256
    assert fc.takes_fused_iteration(2 * fc.NB_STRIDE, 5, 2) and 2 * fc.NB_STRIDE > fc.SMALL_N
    assert fc.red_blocks_for(2 * fc.NB_STRIDE) == 35
    ptr, dofs = fc.window_patches(fc.NB, 2, 7, 300, 3)
    assert ptr[-1] == len(dofs) == 300 * 14 and dofs.max() < 2 * fc.NB and dofs.min() >= 10
