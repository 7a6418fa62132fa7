"""solver_type allu on the host side (alfi/solver.py:346-352, 414): the fieldsplit_0_lu dictionary key for key, the outer
dictionary around it, and the solver-type validation of HipNavierStokesSolver / DistNavierStokesSolver, which must finish
before any device work (no GPU needed)."""
import pytest

from alfi_amd import nssolver
from alfi_amd.problem import TwoDimLidDrivenCavityProblem


def test_fieldsplit_0_lu_is_the_references_dictionary():
    from alfi_amd.solver import fieldsplit_0_lu
    assert fieldsplit_0_lu() == {"ksp_type": "preonly", "ksp_max_it": 1, "pc_type": "lu",
                                 "pc_factor_mat_solver_type": "mumps", "mat_mumps_icntl_14": 150}
    assert fieldsplit_0_lu(use_mkl=True) == {"ksp_type": "preonly", "ksp_max_it": 1, "pc_type": "lu",
                                             "pc_factor_mat_solver_type": "mkl_pardiso", "mat_mumps_icntl_14": 150}
    import alfi_amd
    assert alfi_amd.fieldsplit_0_lu is fieldsplit_0_lu


@pytest.mark.parametrize("tdim", [2, 3])
def test_outer_solver_around_fieldsplit_0_lu(tdim):
    from alfi_amd.solver import fieldsplit_0_lu, is_fieldsplit_0_lu, outer_solver, fieldsplit_0_mg, mg_levels_solver
    p = outer_solver(tdim, fieldsplit_0_lu())
    assert p["ksp_type"] == "fgmres" and p["pc_type"] == "fieldsplit" and p["pc_fieldsplit_type"] == "schur"
    assert p["pc_fieldsplit_schur_factorization_type"] == "full" and p["pc_fieldsplit_schur_precondition"] == "user"
    assert p["fieldsplit_0"] == fieldsplit_0_lu()
    assert p["fieldsplit_1"]["pc_python_type"].endswith("DGMassInv")
    assert is_fieldsplit_0_lu(p["fieldsplit_0"])
    assert not is_fieldsplit_0_lu(fieldsplit_0_mg(mg_levels_solver(tdim)))


class _NoDevice(Exception):
    pass


@pytest.fixture
def no_device(monkeypatch):
    """Any device context, library load or hierarchy build fails the test: validation must come first."""
    from alfi_amd import hip, _lib

    def boom(*a, **k):
        raise _NoDevice("device work before the solver-type validation")
    monkeypatch.setattr(hip.Context, "__init__", boom)
    monkeypatch.setattr(_lib, "load", boom)
    monkeypatch.setattr(nssolver, "build_hierarchy", boom)
    return boom


@pytest.mark.parametrize("solver_type,reason", [("lu", "pivoting"), ("simple", "algebraic multigrid"),
                                                ("lsc", "algebraic multigrid"), ("alamg", "algebraic multigrid")])
def test_unbuilt_solver_types_raise_not_implemented(no_device, solver_type, reason):
    with pytest.raises(NotImplementedError, match=reason):
        nssolver.HipNavierStokesSolver(TwoDimLidDrivenCavityProblem(4), 1, 2, solver_type=solver_type)


@pytest.mark.parametrize("solver_type", ["ALMG", "mg", "", "allu "])
def test_unknown_solver_type_raises_value_error(no_device, solver_type):
    with pytest.raises(ValueError, match="solver_type"):
        nssolver.HipNavierStokesSolver(TwoDimLidDrivenCavityProblem(4), 1, 2, solver_type=solver_type)


@pytest.mark.parametrize("solver_type", ["almg", "allu"])
def test_built_solver_types_pass_validation(no_device, solver_type):
    # validation passes; the next step (the hierarchy) is device-free here but stubbed to prove the order
    with pytest.raises(_NoDevice):
        nssolver.HipNavierStokesSolver(TwoDimLidDrivenCavityProblem(4), 1, 2, solver_type=solver_type)


def test_partitioned_solver_refuses_allu_before_any_collective(no_device):
    from alfi_amd.dist import DistNavierStokesSolver as cls
    with pytest.raises(NotImplementedError, match="single-rank"):
        cls(TwoDimLidDrivenCavityProblem(4), 1, 2, solver_type="allu")
    with pytest.raises(NotImplementedError, match="algebraic multigrid"):
        cls(TwoDimLidDrivenCavityProblem(4), 1, 2, solver_type="alamg")
