"""Every kernel that streams a stored row piece of a dense inverse (csrc/row_piece.h) reproduces, bit for bit, what the tree
before the loops were unified computed: tests/golden/row_piece_bits.npz, recorded by scripts/record_row_piece_bits.py on an
MI355X from the commit before the unification and committed unchanged.  -m gpu.

The cases, their inputs (closed formulas in integer arithmetic) and the kernel each one reaches are in the recording script,
which this file imports; case 11 builds its condensed levels from the operators stored in the fixture.  No tolerances: a
change of the summation order of a row -- columns inside a lane, the shuffle tree, the order of the waves -- shows here as a
differing bit."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_row_piece_bits", os.path.join(ROOT, "scripts", "record_row_piece_bits.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)


@pytest.fixture(scope="module")
def golden():
    with np.load(rec.FIXTURE) as z:
        return {k: z[k] for k in z.files}


def _patches_of(got, key, dof):
    """the patches of the case behind ``key`` that hold ``dof``"""
    stem = key.rsplit(".", 1)[0]
    if stem + ".in.ptr" in got:                 # case 11: the stored patches
        ptr, dofs = got[stem + ".in.ptr"], got[stem + ".in.dofs"]
    else:                                       # "c03.bs2": the windows of the case
        name, bs = stem.split(".bs")
        _, _, ptr, dofs = rec.windows_of(name, int(bs))
    return [p for p in range(len(ptr) - 1) if dof in dofs[ptr[p]:ptr[p + 1]]]


def _compare(got, golden, suffix=""):
    assert got, "the case produced nothing"
    for key in sorted(got):
        want = golden[key + suffix]
        a = np.asarray(got[key])
        if np.array_equal(a, want):
            continue
        if a.shape != want.shape:
            pytest.fail("%s: shape %s, recorded %s" % (key + suffix, a.shape, want.shape))
        if key.endswith(".sha"):
            bad = np.flatnonzero((a != want).any(axis=1))
            pytest.fail("%s: the stored inverses of %d patches differ from the recorded ones, first patch %d"
                        % (key + suffix, len(bad), bad[0]))
        bad = np.flatnonzero(a != want)
        i = int(bad[0])
        held = _patches_of(got, key, i)
        print("%s: %d of %d entries differ; first dof %d: got %r (%s), recorded %r (%s)%s"
              % (key + suffix, len(bad), a.size, i, a[i], a[i].tobytes().hex() if a.dtype == np.float64 else "",
                 want[i], want[i].tobytes().hex() if want.dtype == np.float64 else "",
                 "; patches holding it: %s" % held))
        pytest.fail("%s differs from the recorded bits at dof %d" % (key + suffix, i))


@pytest.mark.parametrize("case", sorted(rec.CASES))
def test_case_reproduces_the_recorded_bits(case, golden):
    got = rec.run_cases([case], golden)
    _compare(got, golden)


def test_sweeps_launched_per_wavefront_reproduce_the_recorded_bits(golden):
    """case 10 under ALFI_MULT_PERSISTENT=0 (a fresh process: the library reads the switch once)"""
    got = rec.sweeps_per_wavefront()
    assert sorted(got) == sorted(k for k in golden if k.endswith(rec.PER_WAVEFRONT))
    _compare({k[:-len(rec.PER_WAVEFRONT)]: v for k, v in got.items()}, golden, rec.PER_WAVEFRONT)
