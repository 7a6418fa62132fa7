"""Block right-hand sides in the de-duplicated level product (bsr_spmv_dedup_block_kernel, kernels_block.hip).  -m gpu

The contract needs no tolerance: column c of ``spmv_block`` / ``residual_block`` equals the single call on column c BIT FOR BIT,
at every width the LDS budget gives (Context.set_block_lds_bytes), looped (a budget that does not fit two columns), and with the
batched kernels switched off.  ``spmv_block_width()`` is asserted against the width rule restated in tests/block_dedup_cases.py on
distinct-column counts that NumPy counted (tests/test_block_rhs_dedup.py), so every case shows that the path it means to test
ran; the single product itself is held against SciPy.

Operators: tests/block_dedup_cases.py -- a first row longer than a chunk inside group 0 with one and with three idle waves in the
last workgroup; row starts at lane 0 of a later wave iteration, on chunk and group boundaries and at lane 63, a row across a
group boundary and five chunks, groups of 1024 and of one distinct column, a ragged and an exact last chunk.  Smoother and
cycles: a fresh child process under ALFI_TEST_LARGE_PATHS=1 (tests/gpu_block_dedup_worker.py), where every operator of a small
[P2+FB]^3 hierarchy takes equal chunks, the fix-up launch and the staged gathers, and the smoother its general launch chain."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from alfi_amd import hip
from tests import block_dedup_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -7.25


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.set_block_kernels(True)
    c.set_block_lds_bytes(dc.DEFAULT_LDS_BUDGET)
    c.close()


def _wide(n, extra):
    """a leading dimension above the default one: n rounded up to even, plus an even extra"""
    return ((n + 1) & ~1) + extra


def _single_columns(ctx, fn, X, *more):
    out = np.empty_like(X)
    for c in range(X.shape[1]):
        dy = ctx.vec(X.shape[0])
        fn(*([ctx.vec(M[:, c]) for M in (X,) + more] + [dy]))
        out[:, c] = dy.get()
    return out


def _reference(ctx, dl, A, seed):
    """X, B and the single product / residual of their five columns, the product held against SciPy"""
    n = dl.n
    rng = np.random.default_rng(seed)
    X, B = rng.standard_normal((n, 5)), rng.standard_normal((n, 5))
    y = _single_columns(ctx, dl.spmv, X)
    r = _single_columns(ctx, lambda x, b, out: dl.residual(b, x, out), X, B)
    S = A.to_scipy()
    assert np.abs(y - S @ X).max() < 1e-13 * np.abs(S @ X).max()
    assert np.abs(r - (B - S @ X)).max() < 1e-13 * np.abs(S @ X).max()
    return X, B, y, r


def _check_block_calls(ctx, dl, X, B, y, r, tag):
    """ncol 1 .. 5 and gapped lists with wider, differing leading dimensions: bitwise, nothing else written, X and B unchanged"""
    n = dl.n
    for ncol in (1, 2, 3, 4, 5):
        dX, dB, dY = ctx.mat(X[:, :ncol]), ctx.mat(B[:, :ncol]), ctx.mat(n, ncol)
        dl.spmv_block(dX, dY)
        assert np.array_equal(dY.get(), y[:, :ncol]), (tag, ncol)
        dl.residual_block(dB, dX, dY)
        assert np.array_equal(dY.get(), r[:, :ncol]), (tag, ncol)
        assert np.array_equal(dX.get(), X[:, :ncol]) and np.array_equal(dB.get(), B[:, :ncol]), (tag, ncol)
    ldx, ldb, ldy = _wide(n, 6), _wide(n, 2), _wide(n, 4)
    dX, dB = ctx.mat(X[:, :4], ld=ldx), ctx.mat(B[:, :4], ld=ldb)
    for call, ref in ((lambda Y, cols: dl.residual_block(dB, dX, Y, cols=cols), r), (lambda Y, cols: dl.spmv_block(dX, Y, cols=cols), y)):
        dY = ctx.mat(np.full((n, 4), SENTINEL), ld=ldy)
        call(dY, [0, 2, 3])
        Y = dY.get()
        assert np.array_equal(Y[:, [0, 2, 3]], ref[:, [0, 2, 3]]) and np.all(Y[:, 1] == SENTINEL), tag
        assert np.all(dY._buf.get().reshape(4, ldy)[:, n:] == 0.0), tag       # nothing written between n and ld
        call(dY, [3, 1])                                                      # any order
        Y = dY.get()
        assert np.array_equal(Y[:, [1, 3]], ref[:, [1, 3]]) and np.array_equal(Y[:, [0, 2]], ref[:, [0, 2]]), tag
        assert np.all(dY._buf.get().reshape(4, ldy)[:, n:] == 0.0), tag
    assert np.array_equal(dX.get(), X[:, :4]) and np.array_equal(dB.get(), B[:, :4]), tag


@pytest.mark.parametrize("bs", [2, 3])
@pytest.mark.parametrize("kind,arg", dc.CASES)
def test_block_product_and_residual_are_the_single_ones(ctx, kind, arg, bs):
    A = dc.operator(kind, arg, bs)
    dl = hip.Level(ctx, A, np.zeros(0, dtype=np.int32))
    try:
        width = dc.expected_width(kind, arg, bs)
        assert width >= 2
        assert dl.spmv_block_batched()                                     # on the parent: False, the de-duplicated product loops
        assert dl.spmv_block_width() == width
        X, B, y, r = _reference(ctx, dl, A, bs)
        for on in (True, False):
            ctx.set_block_kernels(on)
            assert dl.spmv_block_batched() == on and dl.spmv_block_width() == (width if on else 0)
            _check_block_calls(ctx, dl, X, B, y, r, (kind, arg, bs, on))
    finally:
        ctx.set_block_kernels(True)
        dl.close()


def test_the_lds_budget_sets_the_width_and_never_the_bits(ctx):
    A = dc.operator("pattern", "ragged", 3)
    dl = hip.Level(ctx, A, np.zeros(0, dtype=np.int32))
    try:
        assert dl.spmv_block_width() == dc.expected_width("pattern", "ragged", 3) == 2
        X, B, y, r = _reference(ctx, dl, A, 7)
        for budget, width in ((2 * 24 * 1024, 2), (2 * 24 * 1024 - 1, 0), (3 * 24 * 1024, 3), (98304, 4), (dc.DEFAULT_LDS_BUDGET, 2)):
            ctx.set_block_lds_bytes(budget)
            assert width == dc.expected_width("pattern", "ragged", 3, budget)
            assert dl.spmv_block_width() == width and dl.spmv_block_batched() == (width >= 2), budget
            _check_block_calls(ctx, dl, X, B, y, r, budget)
    finally:
        ctx.set_block_lds_bytes(dc.DEFAULT_LDS_BUDGET)
        dl.close()


def test_smoother_and_cycles_on_de_duplicated_levels():
    """tests/gpu_block_dedup_worker.py in a fresh process with the thresholds of the large levels lowered to zero"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_block_dedup_worker.py")],
                         env=dict(os.environ, ALFI_TEST_LARGE_PATHS="1"), cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "OK" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
