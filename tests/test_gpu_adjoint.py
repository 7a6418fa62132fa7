"""Adjoint solves of the Navier-Stokes Jacobian on the device (alfi_level_transpose, alfi_amd.adjoint; alfi/solver.py:520-535):
the in-place block transpose bitwise against SciPy's, patch factors of the transposed operator, the residual of the adjoint
system, adjoint gradients against central differences of forward solves, and that an adjoint solve leaves no trace in the
forward continuation.  -m gpu"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from alfi_amd import hip
from alfi_amd.adjoint import LinearFunctional, LoadFunctional, adjoint_rhs
from alfi_amd.nssolver import HipNavierStokesSolver
from alfi_amd.problem import BSR, TwoDimLidDrivenCavityProblem, ThreeDimLidDrivenCavityProblem


def _force(x):
    d = x.shape[1]
    f = np.zeros_like(x)
    for i in range(d):
        f[:, i] = np.sin(np.pi * x[:, (i + 1) % d]) + 0.5 * x[:, i] * x[:, (i + 2) % d]
    return f


def _weight(x):
    w = np.zeros_like(x)
    w[:, 0] = np.cos(0.5 * np.pi * x[:, 1])
    w[:, 1] = 1.0 + x[:, 0] * x[:, 1]
    return w


class _Forced2(TwoDimLidDrivenCavityProblem):
    m = 1.0

    def rhs(self, x, re):
        return self.m * _force(x)


class _Forced3(ThreeDimLidDrivenCavityProblem):
    m = 1.0

    def rhs(self, x, re):
        return self.m * _force(x)


SOLVERS = {
    "pkp0-2d": lambda **kw: HipNavierStokesSolver(TwoDimLidDrivenCavityProblem(4), 1, 2, **kw),
    "pkp0-3d-k1": lambda **kw: HipNavierStokesSolver(ThreeDimLidDrivenCavityProblem(2), 1, 1, **kw),
    "pkp0-3d-k2": lambda **kw: HipNavierStokesSolver(ThreeDimLidDrivenCavityProblem(2), 1, 2, **kw),
    "supg-2d": lambda **kw: HipNavierStokesSolver(TwoDimLidDrivenCavityProblem(4), 1, 2, stabilisation_type="supg", **kw),
    "gls-2d": lambda **kw: HipNavierStokesSolver(TwoDimLidDrivenCavityProblem(4), 1, 2, stabilisation_type="gls",
                                                 stabilisation_weight=0.05, **kw),
    "sv-2d-burman": lambda **kw: HipNavierStokesSolver(TwoDimLidDrivenCavityProblem(2), 2, 2, discretisation="sv",
                                                       stabilisation_type="burman", stabilisation_weight=5e-3, **kw),
    "sv-3d-k3-burman": lambda **kw: HipNavierStokesSolver(ThreeDimLidDrivenCavityProblem(1), 1, 3, discretisation="sv",
                                                          stabilisation_type="burman", stabilisation_weight=5e-3, **kw),
}


def _refresh_at_random_state(s, seed=0):
    """Every level's operator at a non-trivial velocity (Newton linearisation, stabilisation terms included)."""
    rng = np.random.default_rng(seed)
    u = rng.standard_normal(s.n_u)
    u[s.levels[-1].bc_dofs] = 0.0
    s.nu = 0.02
    s._device_states(u)
    if s.gls:
        s._device_winds()
    s._refresh_device(None, 1.0)


def _mirror(rowptr, colidx):
    rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    key = rows.astype(np.int64) * (len(rowptr) - 1) + colidx
    mkey = colidx.astype(np.int64) * (len(rowptr) - 1) + rows
    order = np.argsort(key)
    pos = np.searchsorted(key[order], mkey)
    assert np.array_equal(key[order][pos], mkey)
    return order[pos]


@pytest.mark.parametrize("case", list(SOLVERS))
def test_transpose_is_bitwise_scipy_transpose(case):
    s = SOLVERS[case]()
    try:
        assert s.device_assembly
        _refresh_at_random_state(s)
        groups = 0
        for L, dl in zip(s.levels, s.hmg.mg.levels):
            rp, ci = np.asarray(L.A.rowptr), np.asarray(L.A.colidx)
            v0 = dl.get_values()
            dl.transpose()
            v1 = dl.get_values()
            assert np.array_equal(v1, np.transpose(v0[_mirror(rp, ci)], (0, 2, 1))), (case, L.level)
            S0 = BSR(L.A.nbrows, L.A.nbcols, L.bs, rp, ci, v0).to_scipy().tocsr()
            S1 = BSR(L.A.nbrows, L.A.nbcols, L.bs, rp, ci, v1).to_scipy().tocsr()
            assert (S0.T.tocsr() != S1).nnz == 0
            assert not np.array_equal(v0, v1)          # the operator is not symmetric: the pass did something
            dl.transpose()
            assert np.array_equal(dl.get_values(), v0), (case, L.level)
            groups = max(groups, (dl.nnzb + 63) // 64)
        assert groups >= 4                             # the lane-major layout's multi-group path
    finally:
        s.close()


@pytest.mark.parametrize("case", ["pkp0-2d", "sv-2d-burman"])
def test_patch_inverses_follow_the_transpose(case):
    s = SOLVERS[case]()
    try:
        _refresh_at_random_state(s, seed=1)
        checked = 0
        for L, dl, obj in zip(s.levels, s.hmg.mg.levels, s.hmg.pc_objs):
            if obj is None or L.level == 0:
                continue
            dl.set_patch_groups(None)                  # dense inverses (the condensed factors hold none to compare)
            dl.factor()
            ptr = np.asarray(obj.patch_ptr)
            ps = np.unique(np.linspace(0, len(ptr) - 2, 12).astype(int))
            fwd = [dl.patch_inverse(p, int(ptr[p + 1] - ptr[p])) for p in ps]
            dl.transpose()
            dl.factor_with_fallback()
            for p, X in zip(ps, fwd):
                Y = dl.patch_inverse(p, int(ptr[p + 1] - ptr[p]))
                assert np.abs(Y - X.T).max() <= 1e-10 * np.abs(X).max(), (case, L.level, p)
                checked += 1
        assert checked > 0
    finally:
        s.close()


def _forward_jacobian(s, adv):
    """[[A, B^T], [B, 0]] of the finest level at the current state, A from a forward refresh (device) or the host pass."""
    import scipy.sparse as sp
    L = s.levels[-1]
    if s.device_assembly:
        s._refresh_device(None, adv)
        vals = s.hmg.mg.levels[-1].get_values()
    else:
        vals = s.level_values(L, s.u.reshape(-1, L.bs), adv, True)
    A = BSR(L.A.nbrows, L.A.nbcols, L.bs, L.A.rowptr, L.A.colidx, vals).to_scipy()
    return sp.bmat([[A, s.B.T], [s.B, None]]).tocsr()


RESIDUAL_CASES = [("pkp0-2d", True, False), ("pkp0-2d", False, False), ("pkp0-3d-k1", True, False), ("supg-2d", True, True),
                  ("gls-2d", True, False), ("sv-2d-burman", True, False), ("sv-2d-burman", False, False)]


@pytest.mark.parametrize("case,dev,forced", RESIDUAL_CASES,
                         ids=["%s-%s%s" % (c, "device" if d else "host", "-force" if f else "") for c, d, f in RESIDUAL_CASES])
def test_adjoint_residual(case, dev, forced):
    s = SOLVERS[case](device_assembly=dev)
    if forced:
        s.problem.__class__ = _Forced3 if s.problem.dim == 3 else _Forced2
    try:
        for re in (10.0, 50.0):
            _, info = s.solve(re)
            assert info["converged"]
        rng = np.random.default_rng(3)
        J = LinearFunctional(LoadFunctional(_weight if s.problem.dim == 2 else _force).gradient(s, s.u, s.p)[0],
                             rng.standard_normal(s.n_p) + 0.2)
        s.setup_adjoint(J)
        info = s.solver_adjoint.solve(rtol=1e-10, atol=0.0)
        assert info["converged"] and info["linear_iter"] > 0, info
        lam = np.concatenate(s.z_adj)
        g = adjoint_rhs(*J.gradient(s, s.u, s.p), s.levels[-1].bc_dofs, s.n_p, s.vol if s.nullspace else None)
        K = _forward_jacobian(s, 1.0)
        r = K.T @ lam - g
        # the device solved with exactly J^T: its own true residual is the one of the forward Jacobian's transpose ...
        rr, gn = np.linalg.norm(r), np.linalg.norm(g)
        assert abs(rr - info["residual_norm"]) <= 1e-2 * rr + 1e-14 * gn, (case, rr, info["residual_norm"])
        # ... and small (FGMRES stops on its recurrence residual: at rtol 1e-10 the true one is 2e-9 .. 1.3e-6 of |g| here)
        assert rr <= 1e-5 * gn, (case, rr / gn)
        assert np.all(s.z_adj[0][s.levels[-1].bc_dofs] == 0.0)
        assert abs(s.vol @ s.z_adj[1]) <= 1e-12 * np.abs(s.z_adj[1]).max() * s.area
    finally:
        s.close()


GRAD_CASES = [("pkp0-2d", 1e-5), ("supg-2d", 1e-5), ("sv-2d-burman", 1e-5), ("pkp0-3d-k1", 1e-4)]


@pytest.mark.parametrize("case,tol", GRAD_CASES, ids=[c[0] for c in GRAD_CASES])
def test_adjoint_gradient_against_central_differences(case, tol):
    """dJ/dm = lam . dF/dm for the amplitude m of a body force, against (J(z(m + h)) - J(z(m - h))) / 2h of forward solves."""
    from alfi_amd import _hostlib
    from alfi_amd.mms import load_vector
    s = SOLVERS[case](snes_rtol=1e-11, snes_atol=1e-14)
    s.problem.__class__ = _Forced3 if s.problem.dim == 3 else _Forced2
    L = s.levels[-1]
    u0, p0 = s.u.copy(), s.p.copy()
    res, m0, h = (10.0, 50.0), 0.5, 1e-3
    J = LoadFunctional(_weight if s.problem.dim == 2 else _force)

    def forward(m):
        s.u, s.p = u0.copy(), p0.copy()
        s.problem.m = m
        for re in res:
            _, info = s.solve(re)
            assert info["converged"]
        return J.value(s, s.u, s.p)

    try:
        Jp, Jm = forward(m0 + h), forward(m0 - h)
        forward(m0)
        info = s.solve_adjoint(J, rtol=1e-10, atol=0.0)[1]
        assert info["converged"], info
        lam_u, lam_p = s.z_adj
        # dF/dm: the residual is affine in m -- F_u -= (f, v), and SUPG's strong residual carries the force too
        dF = -load_vector(L.V, _force)
        if s.supg:
            Fs0, Fs1 = np.zeros(s.n_u), np.zeros(s.n_u)
            w = np.ascontiguousarray(s.u.reshape(-1, L.bs))
            _hostlib.supg(L.V, w, s.nu, s.supg_weight, s.supg_magic, F=Fs0)
            _hostlib.supg(L.V, w, s.nu, s.supg_weight, s.supg_magic, F=Fs1, fq=hip.supg_load(L.V, _force))
            dF += Fs1 - Fs0
        dF[L.bc_dofs] = 0.0
        grad = float(lam_u @ dF)
        fd = (Jp - Jm) / (2 * h)
        assert abs(grad - fd) <= tol * abs(fd), (case, grad, fd)
    finally:
        s.close()


def test_adjoint_leaves_no_trace():
    """Continuation 10 -> 100 -> 200 with an adjoint solve after every step: the same states, bit for bit, and the same
    Newton / Krylov counts as without."""
    runs = []
    for with_adjoint in (False, True):
        s = SOLVERS["pkp0-2d"]()
        try:
            out = []
            for re in (10.0, 100.0, 200.0):
                _, info = s.solve(re)
                out.append((s.u.copy(), s.p.copy(), info["linear_iter"], info["nonlinear_iter"]))
                if with_adjoint:
                    s.solve_adjoint(LoadFunctional(_weight))
            runs.append(out)
        finally:
            s.close()
    for a, b in zip(*runs):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert a[2:] == b[2:]


def test_refusals():
    ctx = hip.Context(0)
    try:
        # structurally non-symmetric: block (0, 1) without (1, 0)
        vals = np.arange(1.0, 1.0 + 3 * 4).reshape(3, 2, 2)
        A = BSR(2, 2, 2, np.array([0, 2, 3], dtype=np.int32), np.array([0, 1, 1], dtype=np.int32), vals)
        lv = hip.Level(ctx, A, np.zeros(0, dtype=np.int32))
        with pytest.raises(hip.AlfiHipError, match="error -2"):
            lv.transpose()
        assert np.array_equal(lv.get_values(), vals)
        with pytest.raises(hip.AlfiHipError, match="error -2"):
            lv.transpose()
        assert np.array_equal(lv.get_values(), vals)
        lv.close()
        # the symmetric pattern of the same size transposes
        vals = np.arange(1.0, 1.0 + 4 * 4).reshape(4, 2, 2)
        A = BSR(2, 2, 2, np.array([0, 2, 4], dtype=np.int32), np.array([0, 1, 0, 1], dtype=np.int32), vals)
        lv = hip.Level(ctx, A, np.zeros(0, dtype=np.int32))
        lv.transpose()
        assert np.array_equal(lv.get_values(), np.transpose(vals[[0, 2, 1, 3]], (0, 2, 1)))
        lv.close()
    finally:
        ctx.close()
    s = SOLVERS["pkp0-2d"]()
    try:
        with pytest.raises(RuntimeError, match="before any solve"):
            s.solve_adjoint(LoadFunctional(_weight))
    finally:
        s.close()
