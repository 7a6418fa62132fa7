"""Which levels take the early-load form of the condensed apply's front kernel: the rule of csrc/cond_layout.h
(cond_ahead) against its long-hand statement, and the waves of the front workgroup.  CPU only."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "alfi_amd", "csrc")


@pytest.mark.parametrize("flags", [(), ("-DALFI_COND_AHEAD=0",)], ids=["library", "ab-build"])
def test_truth_table_of_the_rule(tmp_path, flags):
    """tests/cond_ahead_rule_check.cpp: max_m 15 / 16 / 17 and max_pairs 64 / 65 / 128 / 129 / 512 / 513 among others; with
    ALFI_COND_AHEAD=0 (scripts/build_variant.sh) no level takes the form"""
    exe = str(tmp_path / "cond_ahead_rule_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-I", CSRC, *flags,
                           os.path.join(ROOT, "tests", "cond_ahead_rule_check.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.startswith("OK "), r.stdout


def test_the_gpu_test_restates_the_same_rule():
    """tests/test_gpu_cond_ahead.py decides on a host plan which form a level takes"""
    from tests.test_gpu_cond_ahead import takes_ahead
    for m in (15, 16, 17):
        for mp in (64, 65, 128, 129, 512, 513):
            assert takes_ahead({"max_m": m, "max_pairs": mp}) == (m <= 16 and mp <= 512), (m, mp)
