"""The Krylov kernels at their dispatch boundaries (csrc/kernels_vec.hip, driven by alfi_smooth_fgmres in
csrc/api_smoother.hip and alfi_saddle_solve in csrc/api_saddle.hip), against plain FP64 references.  -m gpu

1. The FGMRES(k) smoother on synthetic levels (tests/krylov_reference.py: random, strongly diagonally dominant block
   operators whose patch inverses LAPACK and the device agree on to ~1e-15), so that only the Krylov arithmetic can differ
   from oracle.alfi_oracle.fgmres.  Every case asserts the branch it names by the Python mirror of the dispatch predicates
   and by the profiler's per-level region counts: the fused four-launch iteration (each of the six (bs, LPR) products, one
   to 1024 product partials, partition of unity, odd n), the general chain with the reduction inside the consumer, the
   general chain with separate reductions (passes of 16 vectors for k > 16, n > 1 048 576 where the partials exceed 256,
   n > 4 194 304 where their number is capped and the grid-stride loops make several passes), workspace reuse, b = 0 and
   the refused k.
2. The outer FGMRES of the saddle-point solve against oracle.alfi_oracle.saddle_solve on the same preconditioner (the
   oracle multigrid applies the device's patch, transfer and coarse inverses): fixed iteration counts with restarts,
   stopping on atol, b = 0, restart changed between calls, alfi_saddle_dot at odd and even length.

Measured on an MI355X, relative to the max-norm of the reference; each bound is at most 10 x the largest measured value
(and never looser than 1e-10 for the smoother, 1e-7 for the outer solve):
    smoother, all synthetic cases             8.0e-16 .. 2.44e-15     SMOOTH_TOL  = 2e-14
    outer solve, x (restart 1 .. 30)          5.0e-16 .. 3.23e-15     OUTER_TOL   = 3e-14
    outer solve, true residual norm           3.3e-13 .. 7.95e-9      OUTER_R_TOL = 7e-8
(the residual norm is relative to itself: it ends at 4.6e-9 |b| for restart 30 in 2-D, where its last digits are rounding)
"""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from alfi_amd.problem import TwoDimLidDrivenCavityProblem, ThreeDimLidDrivenCavityProblem
from tests import krylov_reference as KR

SMOOTH_TOL = 2e-14
OUTER_TOL = 3e-14
OUTER_R_TOL = 7e-8


@pytest.fixture(scope="module")
def ctx():
    from alfi_amd import hip
    c = hip.Context(0)
    yield c
    c.close()


def _rows(lo, hi, long=0):
    """Block-row lengths uniform in [lo, hi]; ``long``: one row of that many blocks (the longest row decides the path)."""
    def f(rng, nb):
        r = rng.integers(lo, hi + 1, nb)
        if long:
            r[nb // 2] = long
        return r
    return f


# id: (bs, nodes, row lengths, patch nodes, patch step, partition of unity, ks, path, LPR of the fused product or None)
SMOOTH_CASES = {
    "fused-bs2-lpr4-one-partial": (2, 1000, _rows(2, 10), 1, 1, False, (1, 2, 15), "fused", 4),
    "fused-bs2-lpr4-pou": (2, 1500, _rows(2, 10), 2, 1, True, (1, 2, 15), "fused", 4),
    "fused-bs2-lpr8": (2, 16000, _rows(14, 30), 1, 1, False, (1, 2, 15), "fused", 8),
    "fused-bs2-lpr32-small-n": (2, 5000, _rows(42, 60), 1, 1, False, (1, 2, 15), "fused", 32),
    "fused-bs3-lpr8-odd-pou": (3, 2001, _rows(2, 16), 2, 1, True, (1, 2, 15), "fused", 8),
    "fused-bs3-lpr16-odd": (3, 8001, _rows(26, 32), 1, 1, False, (1, 2, 15), "fused", 16),
    "fused-bs3-lpr32-small-n-odd": (3, 4001, _rows(50, 70), 1, 1, False, (1, 2, 15), "fused", 32),
    "fused-bs2-1e5-782-partials-pou": (2, 50001, _rows(2, 10), 2, 1, True, (1, 2, 15), "fused", 4),
    "fused-bs3-1e5-odd-1024-partials": (3, 33335, _rows(2, 16), 2, 2, False, (1, 2, 15), "fused", 8),
    "fused-bs2-G257": (2, 524290, _rows(2, 6), 1, 1, False, (4,), "fused", 4),
    "general-consumer-bs2": (2, 60000, _rows(2, 8, long=40), 1, 1, False, (1, 15), "general-consumer", None),
    "general-consumer-bs3-odd-pou": (3, 100001, _rows(2, 6, long=40), 2, 1, True, (1, 15), "general-consumer", None),
    "general-separate-k-bs2": (2, 3000, _rows(2, 10), 1, 1, False, (16, 17, 31), "general-separate", None),
    "general-separate-k-bs3-odd": (3, 10001, _rows(2, 10), 2, 1, True, (16, 17, 31), "general-separate", None),
    "general-separate-G257-bs2": (2, 524290, _rows(2, 6, long=40), 1, 1, False, (3, 17), "general-separate", None),
    "general-separate-G1024-bs3-odd": (3, 1398103, _rows(2, 4, long=40), 1, 1, False, (2,), "general-separate", None),
}


def _make(case, seed):
    bs, nb, rows, m, step, pou, ks, path, lpr = SMOOTH_CASES[case]
    rng = np.random.default_rng(seed)
    lev = KR.SyntheticLevel(nb, bs, rows(rng, nb), m=m, step=step, seed=seed)
    return lev, pou, ks, path, lpr


def _smooth(dl, k, b, x0, nonzero):
    ctx = dl.ctx
    db, dx = ctx.vec(b), ctx.vec(x0)
    dl.smooth(k, db, dx, nonzero_guess=nonzero)
    return dx.get()


@pytest.mark.parametrize("case", list(SMOOTH_CASES))
def test_smoother_on_synthetic_levels(ctx, case):
    from oracle import alfi_oracle as O
    lev, pou, ks, path, lpr = _make(case, seed=sorted(SMOOTH_CASES).index(case))
    n = lev.n
    # the case lands on the branch it names
    for k in ks:
        assert KR.smoother_path(n, lev.max_row, k) == path, (k, n, lev.max_row)
    G = KR.red_blocks_for(n)
    if path == "fused":
        assert KR.spmv_dot_lpr(lev.bs, lev.avg) == lpr, lev.avg
        parts = min(math.ceil(lev.nb / (256 // lpr)), KR.RED_BLOCKS)     # partials of the fused product
        if "one-partial" in case:
            assert G == 1                                                 # one norm partial
        if "partials" in case:
            assert parts > 256 and (parts == KR.RED_BLOCKS) == ("1024" in case)
        if "G257" in case:
            assert G == 257
    else:
        if "consumer" in case:
            assert lev.max_row > 32 and KR.SMALL_N < n <= 1048576 and G <= 256
        if "G257" in case:
            assert G == 257
        if "G1024" in case:
            assert n > 4194304 and G == KR.RED_BLOCKS and (n + 1) // 2 > KR.RED_BLOCKS * 256
    assert (n % 2 == 1) == ("odd" in case)
    if pou:
        assert lev.count.max() == 2                                       # overlapping patches: the weights matter
    dl = lev.device_level(ctx, pou)
    M = lev.smoother(pou)
    rng = np.random.default_rng(7)
    b, x0 = rng.standard_normal(n), rng.standard_normal(n)
    worst = 0.0
    ctx.prof_enable(True)
    try:
        for k in ks:
            for nonzero in (True, False):
                ctx.prof_reset()
                got = _smooth(dl, k, b, x0, nonzero)
                prof = ctx.prof_get(dl.id)
                assert (prof["MATMULT"][1], prof["BLAS1"][1]) == KR.smoother_launch_counts(path, k, nonzero), (k, nonzero, prof)
                ref = O.fgmres(lev.matvec, M, b, x0 if nonzero else np.zeros(n), k, nonzero_guess=nonzero)
                e = KR.relerr(got, ref)
                worst = max(worst, e)
                assert e < SMOOTH_TOL, (k, nonzero, e)
    finally:
        ctx.prof_enable(False)
    # b = 0: exactly zero from a zero guess (no 0/0 anywhere on the path)
    kmax = max(ks)
    assert not np.any(_smooth(dl, kmax, np.zeros(n), x0, False))
    assert not np.any(_smooth(dl, kmax, np.zeros(n), np.zeros(n), True))
    print("smoother [%s] n = %d, G = %d, ks = %s: worst rel err %.2e" % (case, n, G, ks, worst))
    dl.close()


def test_smoother_workspace_reuse(ctx):
    """ensure_fgmres_workspace never shrinks: k = 3 and 15 after k = 20 run with the K = 20 Hessenberg layout, and must give
    the bits of the same call on a fresh level (and match the reference)."""
    from oracle import alfi_oracle as O
    lev = KR.SyntheticLevel(2001, 3, np.random.default_rng(3).integers(2, 12, 2001), seed=3)
    M = lev.smoother()
    rng = np.random.default_rng(8)
    b, x0 = rng.standard_normal(lev.n), rng.standard_normal(lev.n)
    dl = lev.device_level(ctx)
    for k in (20, 3, 15):
        got = _smooth(dl, k, b, x0, True)
        fresh = lev.device_level(ctx)
        assert np.array_equal(got, _smooth(fresh, k, b, x0, True)), k
        fresh.close()
        assert KR.relerr(got, O.fgmres(lev.matvec, M, b, x0, k)) < SMOOTH_TOL, k
    dl.close()


def test_smoother_refuses_k_0_and_32(ctx):
    from alfi_amd import hip
    lev = KR.SyntheticLevel(200, 2, np.full(200, 3), seed=4)
    dl = lev.device_level(ctx)
    b = np.ones(lev.n)
    for k in (0, 32):
        with pytest.raises(hip.AlfiHipError):
            _smooth(dl, k, b, b, True)
    fresh = lev.device_level(ctx)
    assert np.array_equal(_smooth(dl, 31, b, b, True), _smooth(fresh, 31, b, b, True))     # the level is still usable
    fresh.close()
    dl.close()


# ---- outer solve -----------------------------------------------------------------------------------------------------------
# gamma = 1e-3 and two smoothing iterations: a weak augmented-Lagrangian preconditioner, so that 40 outer iterations stay far
# above rounding (the test asserts it) and every restart changes the iterate
OUTER = {"2d-P2": (lambda: TwoDimLidDrivenCavityProblem(4), 2, 1),
         "3d-P1FB-odd": (lambda: ThreeDimLidDrivenCavityProblem(2), 1, 1)}
OUTER_KSM, OUTER_GAMMA, OUTER_RE, MAX_IT = 2, 1e-3, 100.0, 40


@pytest.fixture(scope="module", params=list(OUTER))
def outer(request, ctx):
    from alfi_amd import hip
    from alfi_amd.problem import build_hierarchy, build_pressure_coupling
    mk, ke, nref = OUTER[request.param]
    lv, tr = build_hierarchy(mk(), nref, ke, Re=OUTER_RE, gamma=OUTER_GAMMA)
    L = lv[-1]
    Cinv = hip.coarse_inverse(lv[0].A)
    dmg = hip.Multigrid(ctx, lv, tr, OUTER_KSM, robust_restriction=True, coarse_inv=Cinv)
    B, vol = build_pressure_coupling(L)
    saddle = hip.Saddle(dmg, B, vol, L.nu, L.gamma)
    omg = KR.oracle_mg_with_device_inverses(lv, tr, OUTER_KSM, dmg, Cinv, schoeberl_restriction=True)
    rng = np.random.default_rng(12)
    f = rng.standard_normal(L.n)
    f[L.bc_dofs] = 0.0
    g = rng.standard_normal(B.shape[0])
    b = np.concatenate([f, g - g.mean()])
    A = L.A.to_scipy().tocsr()

    def K(x):
        return np.concatenate([A @ x[:L.n] + B.T @ x[L.n:], B @ x[:L.n]])
    yield dict(name=request.param, L=L, A=A, B=B, vol=vol, saddle=saddle, omg=omg, b=b, K=K, n=saddle.n)
    saddle.close()
    dmg.close()


def _oracle(o, **kw):
    from oracle import alfi_oracle as O
    L = o["L"]
    return O.saddle_solve(o["omg"], o["A"], o["B"], o["vol"], L.nu, L.gamma, o["b"], **kw)


def _device(o, **kw):
    ctx = o["saddle"].ctx
    db, dx = ctx.vec(o["b"]), ctx.vec(o["n"])
    its, rn = o["saddle"].solve(db, dx, **kw)
    return dx.get(), its, rn


@pytest.mark.parametrize("restart", [1, 7, 16, 17, 30])
def test_outer_fixed_iterations(outer, restart):
    """rtol = atol = 0: both sides run exactly MAX_IT iterations (restarts after every `restart`, more than 16 Arnoldi
    vectors for 17 and 30, the final cycle cut short by max_it unless restart divides it)."""
    x, its, rn = _device(outer, rtol=0.0, atol=0.0, max_it=MAX_IT, restart=restart)
    xo, its_o, hist = _oracle(outer, rtol=0.0, atol=0.0, max_it=MAX_IT, restart=restart)
    bn = np.linalg.norm(outer["b"])
    assert its == its_o == MAX_IT
    assert min(hist) > 1e-10 * bn, min(hist) / bn         # the comparison never reaches rounding noise
    rno = np.linalg.norm(outer["b"] - outer["K"](xo))
    ex, er = KR.relerr(x, xo), abs(rn - rno) / rno
    print("outer [%s] restart %d: x %.2e, true residual %.2e (|r|/|b| = %.2e)" % (outer["name"], restart, ex, er, rno / bn))
    assert ex < OUTER_TOL and er < OUTER_R_TOL, (ex, er)


@pytest.mark.parametrize("restart", [7, 30])
def test_outer_stops_on_atol(outer, restart):
    """rtol = 0 and an atol between two entries of the oracle's residual history: the same iteration count."""
    _, _, hist = _oracle(outer, rtol=0.0, atol=0.0, max_it=MAX_IT, restart=restart)
    h = np.array(hist)
    m = next(i for i in range(12, MAX_IT) if h[:i + 1].min() > 1.3 * h[i + 1])
    atol = math.sqrt(h[:m + 1].min() * h[m + 1])
    xo, its_o, _ = _oracle(outer, rtol=0.0, atol=atol, max_it=MAX_IT, restart=restart)
    x, its, rn = _device(outer, rtol=0.0, atol=atol, max_it=MAX_IT, restart=restart)
    assert its_o == m + 1 and its == its_o, (its, its_o, m)
    assert KR.relerr(x, xo) < OUTER_TOL


def test_outer_zero_rhs_restart_changes_and_refusals(outer):
    from alfi_amd import hip
    S, ctx, n = outer["saddle"], outer["saddle"].ctx, outer["n"]
    db, dx = ctx.vec(n), ctx.vec(np.ones(n))
    assert S.solve(db, dx, rtol=0.0, atol=0.0, max_it=MAX_IT, restart=7) == (0, 0.0)
    assert not np.any(dx.get())
    # restart 7 -> 30 -> 7 on one Saddle (V, Z and the Hessenberg reallocated twice): the two 7-runs give the same bits
    r7 = _device(outer, rtol=0.0, atol=0.0, max_it=20, restart=7)
    r30 = _device(outer, rtol=0.0, atol=0.0, max_it=20, restart=30)
    r7b = _device(outer, rtol=0.0, atol=0.0, max_it=20, restart=7)
    assert np.array_equal(r7[0], r7b[0]) and r7[1:] == r7b[1:] and not np.array_equal(r7[0], r30[0])
    for restart in (0, 31):
        with pytest.raises(hip.AlfiHipError):
            _device(outer, restart=restart)


def test_saddle_dot(outer):
    """alfi_saddle_dot (multi_dot_kernel with stride n: the entry-pair kernel at even n, the scalar one at odd n) against
    math.fsum of the products."""
    S, ctx, n = outer["saddle"], outer["saddle"].ctx, outer["n"]
    assert (n % 2 == 1) == ("odd" in outer["name"])
    rng = np.random.default_rng(13)
    for _ in range(3):
        x, y = rng.standard_normal(n), rng.standard_normal(n)
        ref = math.fsum(x * y)
        assert abs(S.dot(ctx.vec(x), ctx.vec(y)) - ref) < 1e-14 * math.fsum(np.abs(x * y)), ref
