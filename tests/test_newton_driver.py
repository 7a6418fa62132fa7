"""The Newton driver of alfi_amd.nssolver / alfi_amd.dist_nssolver on the host side (no GPU, the library is never loaded): the
structure of the modules, the semantics of the ONE Newton loop for both kinds of state (host arrays, device-resident) on a
made-up problem, and the order of the collectives when the device-side operator refresh is set up on partitioned levels."""
import os
import subprocess
import sys
import threading
import types
import warnings

import numpy as np
import pytest

from alfi_amd import hip
from alfi_amd.nssolver import HipNavierStokesSolver


# -- structure ----------------------------------------------------------------------------------------------------------------
def test_partitioned_solver_is_a_class_of_its_own_module():
    import alfi_amd.dist
    import alfi_amd.dist_nssolver
    cls = alfi_amd.dist.DistNavierStokesSolver
    assert isinstance(cls, type) and cls is alfi_amd.dist_nssolver.DistNavierStokesSolver
    assert issubclass(cls, HipNavierStokesSolver)
    assert alfi_amd.dist.StateExchange is alfi_amd.dist_nssolver.StateExchange
    assert cls._partitioned is True and HipNavierStokesSolver._partitioned is False
    with pytest.raises(AttributeError):
        alfi_amd.dist.no_such_name


def test_partitioning_alone_loads_neither_the_solver_nor_the_library_nor_torch():
    code = ("import sys, alfi_amd.dist\n"
            "print([m for m in ('alfi_amd.nssolver', 'alfi_amd.dist_nssolver', 'alfi_amd.hip', 'alfi_amd._lib', 'torch') "
            "if m in sys.modules])")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, check=True, cwd=root)
    assert out.stdout.strip() == "[]", out.stdout


# -- the Newton loop on a made-up problem ---------------------------------------------------------------------------------------
# z = (u, p), one entry each: F_u = u^2 + p - 5, F_p = u + p - 3, root (2, 1); J = [[2 u, 1], [1, 1]] depends on u alone, as the
# solver's refresh is handed the velocity alone
def _F(z):
    return np.array([z[0] ** 2 + z[1] - 5.0, z[0] + z[1] - 3.0])


def _J(u):
    return np.array([[2.0 * u, 1.0], [1.0, 1.0]])


Z0 = np.array([3.0, 0.5])


class _Vec(object):
    """Stands for a device vector."""

    def __init__(self, n):
        self.a, self.n = np.zeros(n), n

    def get(self):
        return self.a.copy()


def _stub_solver(kind, **snes):
    """A solver that was never constructed: the set-up of ``solve`` stubbed away, the primitive operations of the state kind
    replaced by the made-up problem.  ``s.log``: the Krylov counts handed out and the current Jacobian."""
    s = HipNavierStokesSolver.__new__(HipNavierStokesSolver)
    s.problem, s.verbose, s.char_L, s.char_U = object(), False, 1.0, 1.0
    s.supg = s.gls = s.burman = s.nullspace = False
    s.device_assembly = kind == "device"
    s.timings = {"assemble_s": 0.0, "factor_s": 0.0, "residual_s": 0.0, "solve_s": 0.0, "newton_steps": 0}
    s.n_u = s.n_p = 1
    s._host_u, s._host_p = Z0[:1].copy(), Z0[1:].copy()
    s._device_newer = s._device_current = False
    s._set_parameters = lambda: None
    s.snes_rtol, s.snes_atol, s.snes_stol, s.snes_max_it = snes["rtol"], snes["atol"], snes["stol"], snes["max_it"]
    s.log = types.SimpleNamespace(its=[], J=None)

    def krylov_its():
        s.log.its.append(3 + len(s.log.its))
        return s.log.its[-1]
    if kind == "host":
        s.residual = lambda u, p, adv: (_F(np.concatenate([u, p]))[:1], _F(np.concatenate([u, p]))[1:])

        def rediscretise(u, adv):
            s.log.J = _J(u[0])

        def linear_solve(rhs):                              # J d = rhs
            d = np.linalg.solve(s.log.J, rhs)
            return d, krylov_its(), 0.0
        s._rediscretise, s._linear_solve = rediscretise, linear_solve
    else:
        s._dz, s._dF, s._dd = _Vec(2), _Vec(2), _Vec(2)

        def push_state():
            s._dz.a[:] = np.concatenate([s._host_u, s._host_p])

        def residual_on_device(adv):
            s._dF.a[:] = _F(s._dz.a)

        def rediscretise_device(u, adv):
            assert u is None
            s.log.J = _J(s._dz.a[0])

        def zsolve(b, x):                                   # J e = b
            x.a[:] = np.linalg.solve(s.log.J, b.a)
            return krylov_its(), 0.0

        def zaxpy(y, x, a):
            y.a += a * x.a
        s._push_state, s._residual_on_device, s._rediscretise_device = push_state, residual_on_device, rediscretise_device
        s._zsolve, s._zaxpy, s._zdot = zsolve, zaxpy, lambda x, y: float(x.a @ y.a)
    return s


def _solve(kind, **snes):
    s = _stub_solver(kind, **snes)
    z, info = s.solve(100.0)
    u, p = z
    # invariants of every outcome
    assert len(info["residual_history"]) == info["nonlinear_iter"] + 1
    assert info["linear_iter"] == sum(s.log.its) and len(s.log.its) == info["nonlinear_iter"]
    assert s.timings["newton_steps"] == info["nonlinear_iter"]
    assert info["Re"] == 100.0 and info["nu"] == 1.0 / 100.0
    assert info["residual_history"][0] == pytest.approx(np.linalg.norm(_F(Z0)), rel=1e-14)
    assert info["residual_history"][-1] == pytest.approx(np.linalg.norm(_F(np.array([u[0], p[0]]))), rel=1e-14, abs=1e-300)
    assert u is s.u and p is s.p
    return s, np.array([u[0], p[0]]), info


KINDS = ["host", "device"]


@pytest.mark.parametrize("kind", KINDS)
def test_newton_stops_on_the_residual_norm(kind):
    rtol, atol = 1e-10, 1e-13
    s, z, info = _solve(kind, rtol=rtol, atol=atol, stol=0.0, max_it=20)
    h = info["residual_history"]
    tol = max(rtol * h[0], atol)
    assert info["converged"] and info["converged_reason"] == "FNORM"
    assert h[-1] <= tol and all(f > tol for f in h[:-1])           # stopped once, and not before, |F| <= max(rtol f0, atol)
    assert 0 < info["nonlinear_iter"] < 20
    assert np.allclose(z, [2.0, 1.0], atol=1e-9)
    # ... and on the absolute tolerance where that is the larger one
    s, z, info = _solve(kind, rtol=0.0, atol=1e-3, stol=0.0, max_it=20)
    h = info["residual_history"]
    assert info["converged_reason"] == "FNORM" and h[-1] <= 1e-3 and all(f > 1e-3 for f in h[:-1])


@pytest.mark.parametrize("kind", KINDS)
def test_newton_stops_on_a_small_step_first(kind):
    stol = 1e-3
    s, z, info = _solve(kind, rtol=0.0, atol=0.0, stol=stol, max_it=20)
    assert info["converged"] and info["converged_reason"] == "SNORM_RELATIVE"
    assert info["residual_history"][-1] > 0.0                          # the residual test had not fired
    assert 0 < info["nonlinear_iter"] < 20
    # the iterates of Newton's method from Z0, recomputed: the last step, and no earlier one, is below stol |iterate|
    zz, small = Z0.copy(), []
    for _ in range(info["nonlinear_iter"]):
        d = np.linalg.solve(_J(zz[0]), -_F(zz))
        zz = zz + d
        small.append(np.linalg.norm(d) < stol * np.linalg.norm(zz))
    assert small == [False] * (len(small) - 1) + [True]
    assert np.allclose(z, zz, rtol=1e-14, atol=0.0)


@pytest.mark.parametrize("kind", KINDS)
def test_newton_gives_up_after_snes_max_it_steps(kind):
    s, z, info = _solve(kind, rtol=0.0, atol=0.0, stol=0.0, max_it=3)
    assert info["nonlinear_iter"] == 3 and len(info["residual_history"]) == 4
    assert not info["converged"]
    assert s.log.its == [3, 4, 5] and info["linear_iter"] == 12


def test_both_state_kinds_walk_the_same_iterates():
    a = _solve("host", rtol=1e-10, atol=1e-13, stol=1e-6, max_it=20)
    b = _solve("device", rtol=1e-10, atol=1e-13, stol=1e-6, max_it=20)
    assert a[2]["nonlinear_iter"] == b[2]["nonlinear_iter"] and a[2]["converged_reason"] == b[2]["converged_reason"]
    assert np.allclose(a[2]["residual_history"], b[2]["residual_history"], rtol=1e-12, atol=1e-15)
    assert sorted(a[2]) == sorted(b[2]) == sorted(["Re", "nu", "linear_iter", "nonlinear_iter", "time", "residual_history",
                                                   "converged", "converged_reason"])


# -- collective order of the device-assembly set-up on partitioned levels -------------------------------------------------------
class _Comm(object):
    """Two ranks as two threads: ``all_gather_object`` really pairs the n-th call of one rank with the n-th call of the other
    (a rank that calls alone times out), and records what it was given."""

    def __init__(self, barrier, slots, rank):
        self.barrier, self.slots, self.rank, self.calls = barrier, slots, rank, []

    def all_gather_object(self, obj):
        self.calls.append("agree" if isinstance(obj, bool) else "ghost-lists")
        self.slots[self.rank] = obj
        self.barrier.wait()
        out = list(self.slots)
        self.barrier.wait()
        assert len({type(o) for o in out}) == 1, "collectives of different kinds paired up: %r" % (out,)
        return out


def _two_ranks(failing_phase):
    """Rank 0 raises AlfiHipError in phase ``failing_phase`` (1: rank-local, 2: the state exchange, None: nowhere)."""
    from alfi_amd.dist import DistNavierStokesSolver
    barrier, slots = threading.Barrier(2, timeout=10.0), [None, None]
    ranks, errors = [], []
    for rank in range(2):
        s = DistNavierStokesSolver.__new__(DistNavierStokesSolver)
        s.dmg = types.SimpleNamespace(comm=_Comm(barrier, slots, rank))
        s.device_assembly, s._values_on_device, s.entered = True, False, []

        def local(s=s, rank=rank):
            s.entered.append("local")
            if failing_phase == 1 and rank == 0:
                raise hip.AlfiHipError("no refresh here")

        def exchange(s=s, rank=rank):
            s.entered.append("exchange")
            s.dmg.comm.all_gather_object(["ghosts wanted of rank %d" % rank])     # StateExchange's first communication
            if failing_phase == 2 and rank == 0:
                raise hip.AlfiHipError("no exchange level here")
        s._setup_device_assembly, s._setup_state_exchange = local, exchange
        ranks.append(s)

    def run(s):
        try:
            s._start_device_assembly()
        except BaseException as e:          # noqa: BLE001
            errors.append(e)
            barrier.abort()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        threads = [threading.Thread(target=run, args=(s,)) for s in ranks]
        for t in threads:
            t.start()
        for t in threads:
            t.join(30.0)
    assert not errors, errors
    assert not any(t.is_alive() for t in threads)
    return ranks, [str(w.message) for w in caught]


def test_a_rank_failing_in_the_rank_local_phase_meets_the_others_in_the_agreement():
    (bad, good), warned = _two_ranks(1)
    assert bad.dmg.comm.calls == good.dmg.comm.calls == ["agree"]
    assert bad.entered == ["local"] and good.entered == ["local"]           # nobody starts the exchange's collectives
    assert bad.device_assembly is False and good.device_assembly is False
    assert len(warned) == 2 and all("device-side operator refresh not available" in w for w in warned)
    assert sum("no refresh here" in w for w in warned) == 1
    assert sum("another rank failed to set it up" in w for w in warned) == 1


def test_a_rank_failing_in_the_exchange_phase_meets_the_others_in_the_second_agreement():
    (bad, good), warned = _two_ranks(2)
    assert bad.dmg.comm.calls == good.dmg.comm.calls == ["agree", "ghost-lists", "agree"]
    assert bad.entered == good.entered == ["local", "exchange"]
    assert bad.device_assembly is False and good.device_assembly is False
    assert len(warned) == 2 and all("device-side operator refresh not available" in w for w in warned)
    assert sum("no exchange level here" in w for w in warned) == 1


def test_no_failure_keeps_the_device_path_with_one_agreement_per_phase():
    (a, b), warned = _two_ranks(None)
    assert a.dmg.comm.calls == b.dmg.comm.calls == ["agree", "ghost-lists", "agree"]
    assert a.device_assembly is True and b.device_assembly is True and not warned


def test_single_gpu_set_up_runs_the_same_method_without_collectives():
    s = HipNavierStokesSolver.__new__(HipNavierStokesSolver)
    s.device_assembly, s._values_on_device = True, False

    def local():
        raise hip.AlfiHipError("legacy operator layout")
    s._setup_device_assembly = local
    with pytest.warns(UserWarning, match="device-side operator refresh not available \\(legacy operator layout\\)"):
        s._start_device_assembly()
    assert s.device_assembly is False
