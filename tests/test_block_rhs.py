"""CPU checks of block right-hand sides: the host-only arithmetic of csrc/block_cols.h under host sanitizers (a stand-alone
program with its own main), the argument checks of ``matApply`` and of the device-matrix helpers (both raise before anything
touches a device), DGMassInv.matApply against ``apply`` column by column, that header, exports and ctypes table name the
same block entry points, and the list handling of the adjoint: ``setup_adjoint`` / ``gradient`` with one functional or a list,
``adjoint_rhs_block`` column by column against tests/adjoint_restatement.py."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BLOCK_SYMBOLS = ["alfi_ctx_set_block_kernels", "alfi_patch_apply_block_info", "alfi_spmv_block_info", "alfi_patch_apply_block",
                 "alfi_spmv_block", "alfi_residual_block", "alfi_smooth_fgmres_block_info", "alfi_smooth_fgmres_block",
                 "alfi_mg_vcycle_block", "alfi_mg_fcycle_block",
                 "alfi_saddle_mult_block", "alfi_saddle_precond_block", "alfi_saddle_solve_block"]


def test_block_cols_header_under_host_sanitizers(tmp_path):
    """tests/block_cols_check.cpp: chunking, validation, overlap and workspace bookkeeping, -fsanitize=address,undefined"""
    exe = str(tmp_path / "block_cols_check")
    # (the sanitizer runtimes linked statically: the program carries them itself, whatever else the process loads)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "alfi_amd", "csrc"),
                           os.path.join(ROOT, "tests", "block_cols_check.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.startswith("OK "), r.stdout


def test_block_entry_points_are_declared_exported_and_bound():
    from alfi_amd import _lib
    header = open(os.path.join(ROOT, "include", "alfi_hip.h")).read()
    lib = _lib.load()
    for name in BLOCK_SYMBOLS:
        assert "int %s(" % name in header, name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name


def test_device_matrix_helper_checks_its_shape():
    from alfi_amd import hip
    for n, ncol, ld in ((10, 0, None), (10, 2, 8), (10, 2, 11), (11, 2, 11)):
        with pytest.raises(ValueError):
            hip.DeviceMat(None, n, ncol, ld)        # raises before the context is used

    class M(object):
        def __init__(self, n, ncol):
            self.n, self.ncol = n, ncol

    assert hip._block_args(10, None, M(10, 3), M(10, 3))[:3] == (3, None, 3)
    ncol, ptr, nx, keep = hip._block_args(10, [2, 0], M(10, 3), M(10, 3))
    assert (ncol, nx) == (2, 3) and keep.dtype == np.int32 and keep.tolist() == [2, 0]
    for mats in ((M(10, 3), M(10, 2)), (M(10, 3), M(12, 3)), (M(12, 3), M(12, 3))):
        with pytest.raises(ValueError):
            hip._block_args(10, None, *mats)


def test_mat_apply_argument_checks():
    from alfi_amd.solver import check_mat_apply_args
    X, Y = np.zeros((6, 3)), np.zeros((6, 3))
    assert check_mat_apply_args(X, Y, 6) == 3
    assert check_mat_apply_args(np.zeros((6, 1)), np.zeros((6, 1)), 6) == 1
    ro = np.zeros((6, 3))
    ro.setflags(write=False)
    assert check_mat_apply_args(ro, Y, 6) == 3         # X may be read-only

    class Dense(object):                               # the petsc4py shape: a dense Mat hands out its array
        def __init__(self, a):
            self.a = a

        def getDenseArray(self):
            return self.a

    assert check_mat_apply_args(Dense(X), Dense(Y), 6) == 3
    bad = [(X, X), (X, X[:, ::-1]), (np.zeros(6), np.zeros(6)), (X, np.zeros((6, 2))), (np.zeros((5, 3)), np.zeros((5, 3))),
           (np.zeros((6, 0)), np.zeros((6, 0))), (X.astype(np.float32), Y), (X, ro), (Dense(X), Dense(X))]
    for a, b in bad:
        with pytest.raises(ValueError):
            check_mat_apply_args(a, b, 6)


def test_dg_mass_inverse_mat_apply_is_apply_per_column():
    from alfi_amd.solver import DGMassInv

    class PC(object):
        attrs = {"nu": 0.01, "gamma": 1.0e4, "mass_diag": np.random.default_rng(0).uniform(0.5, 2.0, 7)}

        def getAttr(self, k):
            return self.attrs[k]

    pc, obj = PC(), DGMassInv()
    obj.initialize(pc)
    X = np.random.default_rng(1).standard_normal((7, 5))
    Y = np.full((7, 5), np.nan)
    obj.matApply(pc, X, Y)
    for c in range(5):
        y = np.empty(7)
        obj.apply(pc, X[:, c], y)
        assert np.array_equal(Y[:, c], y)
    with pytest.raises(ValueError):
        obj.matApply(pc, X, np.zeros((7, 4)))


def test_setup_adjoint_takes_one_functional_or_a_list():
    """A functional that is not a list keeps today's types; a list or tuple becomes a block of right-hand sides."""
    from alfi_amd.adjoint import AdjointSolver, LinearFunctional, as_functionals, gradient, setup_adjoint

    class Solver(object):
        _partitioned = False

    J1, J2 = LinearFunctional(np.ones(4)), LinearFunctional(np.arange(4.0), np.ones(2))
    s = Solver()
    a = setup_adjoint(s, J1)
    assert isinstance(a, AdjointSolver) and s.solver_adjoint is a and s.J_adj is J1 and a.J is J1
    assert a.functionals == [J1] and a.is_list is False
    for Js in ([J1, J2], (J1, J2), [J1]):
        a = setup_adjoint(s, Js)
        assert a.is_list is True and a.functionals == list(Js) and s.J_adj is Js
    assert as_functionals(J2) == ([J2], False)
    with pytest.raises(ValueError):
        setup_adjoint(s, [])
    s._partitioned = True
    with pytest.raises(NotImplementedError):
        setup_adjoint(s, [J1, J2])
    # gradient: a single adjoint takes no index, a list needs one
    lam = (np.arange(4.0), np.array([2.0, -1.0]))
    v = np.arange(6.0) + 1.0
    want = float(lam[0] @ v[:4] + lam[1] @ v[4:])
    s.z_adj = lam
    assert gradient(s, v) == want and gradient(s, (v[:4], v[4:]), dJ_dm=0.5) == 0.5 + want
    with pytest.raises(ValueError):
        gradient(s, v, index=0)
    s.z_adj = [(np.zeros(4), np.zeros(2)), lam]
    assert gradient(s, v, index=1) == want and gradient(s, v, index=0) == 0.0
    with pytest.raises(ValueError):
        gradient(s, v)


def test_adjoint_rhs_block_column_by_column_against_the_restatement():
    """Column i of adjoint_rhs_block is adjoint_rhs of functional i, and the restatement's direct adjoint solve with it satisfies
    J_F^T lam_i = column i on the velocity rows."""
    import adjoint_restatement as R
    from alfi_amd.adjoint import adjoint_rhs, adjoint_rhs_block
    rs = R.Restatement()
    rng = np.random.default_rng(8)
    u = rs.u0 + 0.1 * rng.standard_normal(rs.n_u)
    u[rs.bc] = rs.u0[rs.bc]
    nu = rs.nu0 / 20.0
    grads = [(rng.standard_normal(rs.n_u), None), (rng.standard_normal(rs.n_u), rng.standard_normal(rs.n_p) + 1.5),
             (np.zeros(rs.n_u), rng.standard_normal(rs.n_p))]
    for vol in (rs.vol, None):
        M = adjoint_rhs_block(grads, rs.bc, rs.n_p, vol)
        assert M.shape == (rs.n_u + rs.n_p, 3)
        for i, (g_u, g_p) in enumerate(grads):
            assert np.array_equal(M[:, i], adjoint_rhs(g_u, g_p, rs.bc, rs.n_p, vol))
    M = adjoint_rhs_block(grads, rs.bc, rs.n_p, rs.vol)
    K = rs.jacobian(u, nu)
    for i, (g_u, g_p) in enumerate(grads):
        lam_u, lam_p, _ = rs.adjoint(u, nu, g_u, g_p)
        r = K.T @ np.concatenate([lam_u, lam_p]) - M[:, i]
        assert np.linalg.norm(r[:rs.n_u]) <= 1e-8 * max(np.linalg.norm(M[:, i]), 1.0)
        assert np.abs(lam_u[rs.bc]).max() == 0.0
