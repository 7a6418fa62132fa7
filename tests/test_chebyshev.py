"""CPU checks around the Chebyshev / W-cycle / CG solver of the reference's grad-div experiment (examples/graddiv/graddiv.py):
the restatement the device path is compared with (tests/chebyshev_restatement.py) is pinned by the Chebyshev polynomial itself
and by the experiment's iteration counts, and the front end's option handling is checked without a device.  The GPU twin is
tests/test_gpu_chebyshev.py."""
import numpy as np
import pytest

from tests import chebyshev_restatement as R

# CG iteration counts of the experiment for gamma = 0 / 1e2 / 1e4 / 1e6 (MAX_IT = the reference's ">200") as a NumPy restatement
# of the solver described in tests/chebyshev_restatement.py gives them (Saad's recurrence, interval (0.1, 1.1) x the largest Ritz
# value of 10 Arnoldi steps, PCMGMCycle_Private, KSPCG on the unpreconditioned norm): columns patch + Schoeberl transfer, patch +
# plain transfers, Jacobi + Schoeberl transfer
CAP = R.MAX_IT
TABLE = {
    ("2d", "patch", True): (8, 11, 12, 12),
    ("2d", "patch", False): (8, 27, CAP, CAP),
    ("2d", "jacobi", True): (9, 42, CAP, CAP),
    ("3d", "patch", True): (12, 13, 14, 14),
    ("3d", "patch", False): (12, 16, 50, CAP),
    ("3d", "jacobi", True): (16, 39, CAP, CAP),
}


def test_chebyshev_is_the_chebyshev_polynomial():
    """k steps from x0 give x* + p_k(M A)(x0 - x*), p_k(t) = T_k((theta - t) / delta) / T_k(theta / delta), built from dense
    matrices by the three-term recurrence: pins the restatement's smoother (recurrence and scaling)."""
    lv, _ = R.hierarchy("2d", 1e4)
    mg = R.multigrid("2d", 1e4)
    L = mg.levels[-1]
    A = L["A"].toarray()
    n = A.shape[0]
    sm = L["smoother"]
    M = np.zeros((n, n))
    for p, inv in enumerate(sm.inv):
        dofs = sm.patch_dofs[sm.patch_ptr[p]:sm.patch_ptr[p + 1]]
        M[np.ix_(dofs, dofs)] += inv
    M[L["bc"], L["bc"]] = 1.0
    emin, emax = mg.bounds[-1]
    theta, delta = 0.5 * (emax + emin), 0.5 * (emax - emin)
    Y = (theta * np.eye(n) - M @ A) / delta
    rng = np.random.default_rng(1)
    b, x0 = rng.standard_normal(n), rng.standard_normal(n)
    xs = np.linalg.solve(A, b)
    e0 = x0 - xs
    Tm, Tk = e0, Y @ e0                      # T_0(Y) e0, T_1(Y) e0
    tm, tk = 1.0, theta / delta              # T_0, T_1 at theta / delta
    for k in range(1, 5):
        if k > 1:
            Tm, Tk = Tk, 2.0 * (Y @ Tk) - Tm
            tm, tk = tk, 2.0 * (theta / delta) * tk - tm
        want = xs + Tk / tk
        got = R.chebyshev(L["A"], sm.apply, b, x0, k, emin, emax)
        err = np.linalg.norm(got - want) / np.linalg.norm(want)
        assert err <= 1e-10, (k, err)


@pytest.mark.parametrize("case", ["2d", "3d"])
def test_patch_smoother_with_robust_transfer_is_gamma_robust(case):
    its = [R.solve(case, g)[0] for g in R.GAMMAS]
    for got, want in zip(its, TABLE[(case, "patch", True)]):
        assert abs(got - want) <= 1, (its, TABLE[(case, "patch", True)])
    assert max(its) <= 16 and max(its) - min(its) <= 6, its
    for g in R.GAMMAS:
        _, rn, bn = R.solve(case, g)
        assert rn <= 1e-8 * bn


@pytest.mark.parametrize("case,smoother,transfer", [("2d", "patch", False), ("2d", "jacobi", True),
                                                     ("3d", "patch", False), ("3d", "jacobi", True)])
def test_plain_transfers_and_jacobi_are_not(case, smoother, transfer):
    want = TABLE[(case, smoother, transfer)]
    its = [R.solve(case, g, smoother, transfer)[0] for g in R.GAMMAS]
    for got, ref in zip(its, want):
        assert abs(got - ref) <= 1, (its, want)
    if want[2] == CAP:
        assert its[2] > 100, its


def test_graddiv_solver_has_the_reference_keys():
    from alfi_amd.solver import graddiv_solver
    sp = graddiv_solver()
    assert (sp["ksp_type"], sp["ksp_rtol"], sp["ksp_atol"], sp["ksp_max_it"]) == ("cg", 1e-8, 0, 200)
    assert sp["ksp_norm_type"] == "unpreconditioned" and sp["mat_type"] == "aij" and sp["snes_type"] == "ksponly"
    assert sp["pc_type"] == "mg" and sp["pc_mg_cycle_type"] == "w"
    assert sp["mg_coarse_ksp_type"] == "preonly" and sp["mg_coarse_assembled_pc_type"] == "lu"
    mgl = sp["mg_levels"]
    assert mgl["ksp_type"] == "chebyshev" and mgl["ksp_max_it"] == 2
    assert mgl["pc_type"] == "python" and mgl["pc_python_type"] == "alfi_amd.HipPatchPC"
    assert mgl["patch_pc_patch_construct_type"] == "star" and mgl["patch_pc_patch_construct_dim"] == 0
    assert mgl["patch_pc_patch_sub_mat_type"] == "dense" and mgl["patch_sub_pc_type"] == "lu"
    assert mgl["patch_pc_patch_multiplicative"] is False and mgl["patch_pc_patch_partition_of_unity"] is False
    macro = graddiv_solver("patch", patch="macro")["mg_levels"]
    assert macro["patch_pc_patch_construct_python_type"] == "alfi_amd.MacroStar"
    assert macro["patch_pc_patch_sub_mat_type"] == "aij" and macro["patch_sub_pc_factor_mat_solver_type"] == "umfpack"
    jac = graddiv_solver("jacobi")["mg_levels"]
    assert jac == {"ksp_type": "chebyshev", "ksp_max_it": 2, "pc_type": "jacobi"}
    with pytest.raises(NotImplementedError):
        graddiv_solver("amg")


def test_option_parsing_needs_no_device():
    from alfi_amd.solver import HipMG, graddiv_solver, parse_mg_options, fieldsplit_0_mg, mg_levels_solver
    o = parse_mg_options(graddiv_solver())
    assert (o["smoother"], o["k"], o["pc"], o["cycle"], o["full"]) == ("chebyshev", 2, "python", "w", False)
    assert o["esteig"] == (0.0, 0.1, 0.0, 1.1) and o["esteig_steps"] == 10 and o["eigenvalues"] is None
    o = parse_mg_options(fieldsplit_0_mg(mg_levels_solver(2)))            # today's dictionary reads as before
    assert (o["smoother"], o["k"], o["pc"], o["cycle"], o["full"]) == ("fgmres", 6, "python", "v", True)
    sp = graddiv_solver()
    sp["mg_levels"]["ksp_type"] = "richardson"
    with pytest.raises(NotImplementedError, match="fgmres, chebyshev"):
        HipMG(None, [], [], sp)
    for bad in ("1.0", "a,b", "2.0,1.0", "0,1", "1,2,3"):
        sp = graddiv_solver()
        sp["mg_levels"]["ksp_chebyshev_eigenvalues"] = bad
        with pytest.raises(ValueError):
            HipMG(None, [], [], sp)
    sp = graddiv_solver()
    sp["mg_levels"]["ksp_chebyshev_eigenvalues"] = "0.3,3.3"
    assert parse_mg_options(sp)["eigenvalues"] == (0.3, 3.3)
    sp["pc_mg_cycle_type"] = "f"
    with pytest.raises(NotImplementedError):
        parse_mg_options(sp)
