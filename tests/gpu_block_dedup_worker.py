"""Worker of tests/test_gpu_block_rhs_dedup.py::test_smoother_and_cycles_on_de_duplicated_levels, started with
ALFI_TEST_LARGE_PATHS=1: every operator of the 3-D [P2+FB]^3 lid-driven cavity hierarchy (two refinements) takes equal chunks, the
fix-up launch and the de-duplicated gathers, the smoother its general launch chain.  Every level whose operator has at least 1024
blocks must report the batched product at the width of the restated rule; ``smooth_block`` (k = 1 and 10, with and without an
initial guess) and ``vcycle_block`` / ``fcycle_block`` for 5 columns and a gapped list must equal the single calls bit for bit,
with the batched kernels on and off.  Prints ``OK``."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SENTINEL = -7.25


def main():
    assert os.environ.get("ALFI_TEST_LARGE_PATHS") == "1"
    from alfi_amd import hip
    from alfi_amd.problem import ThreeDimLidDrivenCavityProblem, build_hierarchy
    from tests import block_dedup_cases as dc
    ctx = hip.Context(0)
    lv, tr = build_hierarchy(ThreeDimLidDrivenCavityProblem(2), 2, 2, Re=100.0)
    mg = hip.Multigrid(ctx, lv, tr, 2)
    rng = np.random.default_rng(21)
    large = 0
    for L, dl in zip(lv, mg.levels):
        if L.A.nnzb < dc.SPMV_WG:
            continue
        large += 1
        width = dc.block_dedup_width(max(dc.group_distinct(L.A.colidx)), L.A.bs)
        assert width >= 2 and dl.spmv_block_batched() and dl.spmv_block_width() == width, (dl.n, width, dl.spmv_block_width())
    assert large >= 2
    for L, dl in list(zip(lv, mg.levels))[1:]:
        n = dl.n
        assert L.A.nnzb >= dc.SPMV_WG and dl.smooth_block_lockstep(1) and dl.smooth_block_lockstep(10)
        B, X0 = rng.standard_normal((n, 5)), rng.standard_normal((n, 5))
        B[L.bc_dofs] = 0.0
        X0[L.bc_dofs] = 0.0
        for k in (1, 10):
            for guess in (False, True):
                ref = np.empty((n, 5))
                for c in range(5):
                    db, dx = ctx.vec(B[:, c]), ctx.vec(X0[:, c])
                    dl.smooth(k, db, dx, nonzero_guess=guess)
                    ref[:, c] = dx.get()
                assert np.isfinite(ref).all() and np.abs(ref).max() > 0.0
                for on in (True, False):
                    ctx.set_block_kernels(on)
                    assert dl.spmv_block_batched() == on
                    dB, dX = ctx.mat(B), ctx.mat(X0)
                    dl.smooth_block(k, dB, dX, nonzero_guess=guess)
                    assert np.array_equal(dX.get(), ref), (n, k, guess, on)
                    dX = ctx.mat(X0[:, :4], ld=((n + 1) & ~1) + 2)
                    dl.smooth_block(k, ctx.mat(B[:, :4]), dX, nonzero_guess=guess, cols=[0, 2, 3])
                    got = dX.get()
                    assert np.array_equal(got[:, [0, 2, 3]], ref[:, [0, 2, 3]]) and np.array_equal(got[:, 1], X0[:, 1]), (n, k, guess, on)
                ctx.set_block_kernels(True)
    n = lv[-1].n
    B = rng.standard_normal((n, 5))
    B[lv[-1].bc_dofs] = 0.0
    refv, reff = np.empty_like(B), np.empty_like(B)
    for c in range(5):
        db, dx = ctx.vec(B[:, c]), ctx.vec(n)
        mg.vcycle(db, dx)
        refv[:, c] = dx.get()
        mg.fcycle(db, dx)
        reff[:, c] = dx.get()
    assert np.isfinite(refv).all() and np.isfinite(reff).all() and np.abs(refv).max() > 0.0
    for on in (True, False):
        ctx.set_block_kernels(on)
        dB, dX = ctx.mat(B), ctx.mat(n, 5)
        mg.vcycle_block(dB, dX)
        assert np.array_equal(dX.get(), refv), on
        mg.fcycle_block(dB, dX)
        assert np.array_equal(dX.get(), reff), on
        for cycle, ref in ((mg.vcycle_block, refv), (mg.fcycle_block, reff)):
            X0 = np.full((n, 5), SENTINEL)
            X0[:, [0, 2, 4]] = 0.0                                      # (a V-cycle starts from what x holds)
            dX = ctx.mat(X0, ld=((n + 1) & ~1) + 4)
            cycle(dB, dX, cols=[4, 0, 2])
            got = dX.get()
            assert np.array_equal(got[:, [0, 2, 4]], ref[:, [0, 2, 4]]) and np.all(got[:, [1, 3]] == SENTINEL), on
    ctx.set_block_kernels(True)
    mg.close()
    ctx.close()
    print("OK", flush=True)


if __name__ == "__main__":
    main()
