"""2-D Scott-Vogelius [P3]^2-P2dg on the GPU (-m gpu): the shapes the cubic triangle brings through the library for the first
time -- the <2, 10> element kernels, Burman tables with nloc = 10 / nu = 16, macro stars of 146 dofs (register-resident /
matrix-core inversion, one-wave apply) and of 194 (the large-patch path; union-jack mesh), 92-dof transfer blocks, condensed
factors with 20-dof groups, 6 x 6 pressure mass blocks -- each against the reference the existing test of the same quantity
uses, at that test's tolerance (named in every docstring).  Smallest shapes: ldc2d N = 2, nref <= 2; union-jack at nref 1."""
import os
import socket
import subprocess
import sys
import time
from fractions import Fraction

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import exact_cases as C
from tests.sv_p3_2d_cases import PROBLEMS, hierarchy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = (2, 3, False)
WEIGHT = 5e-3


def relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.fixture(scope="module")
def ctx():
    from alfi_amd import hip
    c = hip.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("ncell", [1, 2])
def test_device_operator_terms_are_exact(ctx, ncell):
    """tests/test_gpu_exact_pins.py::test_device_operator_terms_are_exact for (2, "P3"), 1e-12: element_cell_kernel<2, 10, 0>
    and the matrix-free <2, 10, 1> against exact rational integration."""
    from tests.test_gpu_exact_pins import _dense, _level
    mesh, V = C.build_space(2, ARGS, ncell)
    nu, gamma, adv = Fraction(3, 70), Fraction(1250, 3), Fraction(3, 4)
    w = C.rational_field(2, V)
    wf = np.array([[float(x) for x in r] for r in w])
    L, rowptr, colidx = _level(ctx, V)
    st = ctx.vec(wf.ravel())
    for a_ in (adv, Fraction(0)):
        exact = C.exact_operator(2, "P3", ncell, V, nu, gamma, a_, w)
        L.assemble(float(nu), float(gamma), float(a_), st if a_ else None, False)
        got = _dense(V, rowptr, colidx, L.get_values())
        assert np.abs(got - exact).max() < 1e-12 * np.abs(exact).max(), (ncell, float(a_))
        x = np.random.default_rng(2).standard_normal(V.num_nodes * 2)
        dx, dy = ctx.vec(x), ctx.vec(V.num_nodes * 2)
        L.assemble_mult(float(nu), float(gamma), float(a_), st if a_ else None, dx, dy)
        ref = exact @ x
        assert np.abs(dy.get() - ref).max() < 1e-12 * np.abs(ref).max(), (ncell, float(a_))
    L.close()


@pytest.mark.parametrize("gamma", [0.0, 1e4])
@pytest.mark.parametrize("mesh,nref,largest", [("ldc2d", 2, 146), ("unionjack", 1, 194)])
def test_patch_inverses(ctx, mesh, nref, largest, gamma):
    """Dense inverses of every macro star of the finest level against np.linalg.inv.  gamma = 0 (nu K + N(w): patch matrices of
    condition ~1e3): 1e-11 up to 160 dofs and 1e-10 above, the tolerances of tests/test_gpu_parity.py::
    test_patch_sizes_1_to_160_all_row_piece_combinations / test_large_patches.  gamma = 1e4 at Re 100 (the operator of the
    solver: condition 2.4e7, so cond * eps = 5e-9): 1e-8, the tolerance of the patch-inverse test on level operators,
    tests/test_gpu_burman.py::test_patch_inverses_follow_the_pcpatch_facet_rule."""
    from alfi_amd import hip
    lv, _ = hierarchy(mesh, nref, 100.0, gamma)
    L = lv[-1]
    S = L.A.to_scipy().tocsr()
    dl = hip.Level(ctx, L.A, L.bc_dofs)
    dl.set_patches(L.patch_ptr, L.patch_dofs)
    dl.factor()
    sizes = np.diff(L.patch_ptr)
    assert sizes.max() == largest
    compared = set()
    for p in range(len(sizes)):
        dofs = L.patch_dofs[L.patch_ptr[p]:L.patch_ptr[p + 1]]
        ref = np.linalg.inv(S[dofs][:, dofs].toarray())
        tol = 1e-8 if gamma else (1e-11 if sizes.max() <= 160 else 1e-10)
        err = relerr(dl.patch_inverse(p, int(sizes[p])), ref)
        assert err < tol, (p, int(sizes[p]), err)
        compared.add(int(sizes[p]))
    assert 146 in compared and (mesh != "unionjack" or 194 in compared)
    x = np.random.default_rng(0).standard_normal(L.n)
    dx, dy = ctx.vec(x), ctx.vec(L.n)
    dl.patch_apply(dx, dy)
    from oracle import alfi_oracle as O
    ref = O.PatchSmoother(S, L.patch_ptr, L.patch_dofs, L.bc_dofs).apply(x)
    assert relerr(dy.get(), ref) < 1e-7                                 # tests/test_gpu_condensed.py: dense apply against the oracle
    dl.close()


def test_transfers_and_cycles_match_oracle(ctx):
    """tests/test_gpu_sv.py::test_sv_transfers_and_cycles_match_oracle for [P3]^2: Re 100, gamma 1e4, robust restriction on and
    off; prolong / restrict (92-dof macro-cell blocks through the patch kernels) 1e-7, V- and F-cycle 1e-5."""
    from alfi_amd import hip
    from oracle import alfi_oracle as O
    lv, tr = hierarchy("ldc2d", 2, 100.0, 1e4)
    assert tr[0].blk_dofs.shape[1] == 92
    rng = np.random.default_rng(0)
    for robust in (True, False):
        mg = hip.Multigrid(ctx, lv, tr, 3, robust_restriction=robust)
        omg = O.build_oracle_mg(lv, tr, 3, schoeberl_restriction=robust)
        for l in range(1, len(lv)):
            uc = rng.standard_normal(lv[l - 1].n)
            uc[lv[l - 1].bc_dofs] = 0
            rf = rng.standard_normal(lv[l].n)
            duc, dxf, drf, drc = ctx.vec(uc), ctx.vec(lv[l].n), ctx.vec(rf), ctx.vec(lv[l - 1].n)
            mg.transfers[l - 1].prolong(duc, dxf)
            assert relerr(dxf.get(), omg.prolong(l, uc)) < 1e-7
            mg.transfers[l - 1].restrict(drf, drc, robust=robust)
            assert relerr(drc.get(), omg.restrict(l, rf)) < 1e-7
        L = lv[-1]
        b = rng.standard_normal(L.n)
        b[L.bc_dofs] = 0
        db, dx = ctx.vec(b), ctx.vec(L.n)
        mg.vcycle(db, dx)
        assert relerr(dx.get(), omg.vcycle(len(lv) - 1, b, np.zeros(L.n))) < 1e-5
        mg.fcycle(db, dx)
        assert relerr(dx.get(), omg.fcycle(b)) < 1e-5
        mg.close()


def test_outer_solve_matches_oracle(ctx):
    """tests/test_gpu_sv.py::test_sv_outer_solve_matches_oracle for [P3]^2-P2dg (6 x 6 blocks in the CSR mass inverse), 6
    smoothing steps: iteration count within 1 of the oracle's, residual <= 2e-9 |rhs|, velocity within 1e-6."""
    from alfi_amd import hip
    from alfi_amd.sv import build_sv_pressure_coupling
    from oracle import alfi_oracle as O
    lv, tr = hierarchy("ldc2d", 2, 10.0, 1e4)
    L = lv[-1]
    B, M, Minv = build_sv_pressure_coupling(L)
    assert B.shape[0] == 6 * L.V.mesh.num_cells
    b = np.random.default_rng(1).standard_normal(L.n)
    b[L.bc_dofs] = 0
    rhs = np.concatenate([b, np.zeros(B.shape[0])])
    omg = O.build_oracle_mg(lv, tr, 6, schoeberl_restriction=False)
    xo, its_o, hist = O.saddle_solve(omg, omg.levels[-1]["A"], B, None, L.nu, L.gamma, rhs, rtol=1e-9, atol=1e-12, mass_inv=Minv)
    mg = hip.Multigrid(ctx, lv, tr, 6, robust_restriction=False)
    sad = hip.Saddle(mg, B, None, L.nu, L.gamma, remove_constant_nullspace=True, mass_inv=Minv)
    db, dx = ctx.vec(rhs), ctx.vec(L.n + B.shape[0])
    its, rn = sad.solve(db, dx, 1e-9, 1e-12, 500, 30)
    x = dx.get()
    print("outer solve: %d iterations (oracle %d), residual %.2e |rhs|, velocity error %.2e"
          % (its, its_o, rn / np.linalg.norm(rhs), relerr(x[:L.n], xo[:L.n])))
    assert abs(its - its_o) <= 1, (its, its_o)
    assert rn <= 2e-9 * np.linalg.norm(rhs)
    assert relerr(x[:L.n], xo[:L.n]) < 1e-6
    sad.close()
    mg.close()


@pytest.mark.parametrize("mesh,nref", [("ldc2d", 2), ("unionjack", 1)])
def test_condensed_apply_equals_dense_inverse_apply(ctx, mesh, nref):
    """tests/test_gpu_condensed.py::test_condensed_apply_equals_dense_inverse_apply with 20-dof groups: probe < 1e-7 and no
    flagged patch, dense and condensed against the oracle 1e-7, condensed against dense 1e-8, condensed storage below dense."""
    from alfi_amd import hip
    from oracle import alfi_oracle as O
    lv, _ = hierarchy(mesh, nref, 100.0, 1e4)
    L = lv[-1]
    assert (L.patch_groups >= 0).any() and (L.patch_groups < 0).any()
    x = np.random.default_rng(0).standard_normal(L.n)
    out = {}
    for mode in ("dense", "condensed"):
        dl = hip.Level(ctx, L.A, L.bc_dofs)
        dl.set_patches(L.patch_ptr, L.patch_dofs)
        if mode == "condensed":
            dl.set_patch_groups(L.patch_groups)
        dl.factor()
        worst, flagged, _, _ = dl.patch_check()
        print(mesh, mode, "probe", worst, "flagged", flagged)
        assert 0.0 <= worst < 1e-7 and flagged == 0
        dx, dy = ctx.vec(x), ctx.vec(L.n)
        dl.patch_apply(dx, dy)
        out[mode] = (dy.get(), dl.factor_bytes())
        dl.patch_apply(dx, dy)
        assert np.array_equal(dy.get(), out[mode][0])
        dl.close()
    ref = O.PatchSmoother(L.A.to_scipy().tocsr(), L.patch_ptr, L.patch_dofs, L.bc_dofs).apply(x)
    print(mesh, "dense %.2e condensed %.2e (against the oracle), condensed against dense %.2e, bytes %d / %d"
          % (relerr(out["dense"][0], ref), relerr(out["condensed"][0], ref), relerr(out["condensed"][0], out["dense"][0]),
             out["dense"][1], out["condensed"][1]))
    assert relerr(out["dense"][0], ref) < 1e-7
    assert relerr(out["condensed"][0], ref) < 1e-7
    assert relerr(out["condensed"][0], out["dense"][0]) < 1e-8
    assert out["condensed"][1] < 8 * float((np.diff(L.patch_ptr).astype(np.float64) ** 2).sum())


def _solver(device_assembly=True, nref=2):
    from alfi_amd.nssolver import HipNavierStokesSolver
    return HipNavierStokesSolver(PROBLEMS["ldc2d"](), nref, 3, discretisation="sv", stabilisation_type="burman",
                                 stabilisation_weight=WEIGHT, device_assembly=device_assembly)


def test_burman_device_refresh_and_residual_match_host():
    """tests/test_gpu_burman.py::test_device_refresh_and_residual_match_host for [P3]^2 (nloc = 10, 16-node unions, rules of 3
    and 5 points): 1e-12, bitwise repeatable over scratch sizes."""
    s = _solver()
    try:
        assert s.device_assembly and all(L.facet_coupling for L in s.levels)
        assert s.levels[-1].facets.nu == 16 and [L.n for L in s.levels] == [242, 914, 3554]
        rng = np.random.default_rng(0)
        u = rng.standard_normal(s.n_u)
        u[s.levels[-1].bc_dofs] = 0.0
        s.nu = 0.05
        s._device_states(u)
        winds = [st.get().reshape(-1, 2) for st in s._dstate]
        for L, dl, st, w in zip(s.levels, s.hmg.mg.levels, s._dstate, winds):
            host = s.level_values(L, w, 1.0, True)
            dl.assemble_burman(s.nu, s.gamma, 1.0, st, s.burman_weight, True)
            dev = dl.get_values()
            assert np.abs(dev - host).max() <= 1e-12 * np.abs(host).max(), L.level
            dl.assemble(s.nu, s.gamma, 1.0, st, False)
            dl.burman(s.burman_weight, st, True)
            dl.apply_bc()
            assert np.array_equal(dl.get_values(), dev)
            for scratch in (1 << 16, 1 << 22):
                s.ctx.set_assembly_scratch(scratch)
                dl.assemble_burman(s.nu, s.gamma, 1.0, st, s.burman_weight, True)
                assert np.array_equal(dl.get_values(), dev)
            s.ctx.set_assembly_scratch(24 << 30)
        p = rng.standard_normal(s.n_p)
        Fu_d, Fp_d = s._residual_device(u, p, 1.0)
        s.device_assembly = False
        Fu_h, Fp_h = s.residual(u, p, 1.0)
        s.device_assembly = True
        assert np.abs(Fu_d - Fu_h).max() <= 1e-12 * np.abs(Fu_h).max()
        assert np.abs(Fp_d - Fp_h).max() <= 1e-12 * np.abs(Fp_h).max()
        s.burman = False
        Fu_0, _ = s._residual_device(u, p, 1.0)
        s.burman = True
        assert np.abs(Fu_0 - Fu_d).max() > 1e-6 * np.abs(Fu_d).max()
    finally:
        s.close()


def test_burman_patch_inverses_follow_the_pcpatch_facet_rule():
    """tests/test_gpu_burman.py::test_patch_inverses_follow_the_pcpatch_facet_rule for [P3]^2, 1e-8."""
    from alfi_amd.burman import patch_facet_corrections
    from alfi_amd.problem import BSR
    s = _solver(nref=1)
    try:
        d = 2
        u = np.random.default_rng(5).standard_normal(s.n_u)
        u[s.levels[-1].bc_dofs] = 0.0
        s.nu = 0.05
        s._device_states(u)
        for L, dl, st, obj in zip(s.levels, s.hmg.mg.levels, s._dstate, s.hmg.pc_objs):
            if obj is None:
                continue
            assert not obj.condensed
            dl.assemble_burman(s.nu, s.gamma, 1.0, st, s.burman_weight, True)
            dl.factor()
            A = BSR(L.A.nbrows, L.A.nbcols, d, L.A.rowptr, L.A.colidx,
                    s.level_values(L, st.get().reshape(-1, d), 1.0, True)).to_scipy().tocsr()
            beta, scale = L.facet_beta
            ptr, col, fac, sv_ = patch_facet_corrections(L.V, L.facets, obj.patch_ptr, obj.patch_dofs)
            sizes = np.diff(obj.patch_ptr)
            npatch = len(sizes)
            ncorr = 0
            for p in sorted(set([0, npatch // 2, npatch - 1, int(np.argmax(sizes))])):
                dofs = obj.patch_dofs[obj.patch_ptr[p]:obj.patch_ptr[p + 1]]
                n = dofs.size
                Ap = A[dofs][:, dofs].toarray()
                r0 = obj.patch_ptr[p] // d
                for i in range(n // d):
                    for q in range(ptr[r0 + i], ptr[r0 + i + 1]):
                        ncorr += 1
                        for c in range(d):
                            Ap[i * d + c, col[q] * d + c] -= scale * beta[fac[q]] * sv_[q]
                ref = np.linalg.inv(Ap)
                assert np.abs(dl.patch_inverse(p, n) - ref).max() <= 1e-8 * np.abs(ref).max(), (L.level, p)
            assert ncorr > 0 and sizes.max() == 146
    finally:
        s.close()


def test_flagged_patches_of_a_burman_level_are_repaired_with_the_facet_rule():
    """A macro star of a Burman level that fails the residual probe (one of 441 does at ldc2d baseN 10, nref 1: 1.06e-6 against
    the tolerance 1e-6; cond ~ gamma / nu) is re-inverted by the pivoted LU like on any other level -- from the matrix PCPATCH
    assembles, i.e. with the facet rule applied (patch_repair_kernel).  Forced here for every patch by a probe tolerance no
    inverse reaches (own process: the library reads its switches once; the pattern of tests/test_gpu_condensed.py::
    test_flagged_condensed_factors_are_repaired_in_place).  Inverses against np.linalg.inv at 1e-8 (tests/test_gpu_burman.py)."""
    import re
    env = dict(os.environ, ALFI_PATCH_CHECK_TOL="1e-14", ALFI_PATCH_CHECK_FAIL="1e-6")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_burman_repair_worker.py")], env=env, cwd=ROOT,
                         capture_output=True, text=True, timeout=300)
    m = re.search(r"REPAIR (\d+) (\d+) (\S+) (\S+) ERR (\S+) PLAIN (\S+) NPATCH (\d+)", out.stdout)
    assert out.returncode == 0 and m, out.stdout[-2000:] + out.stderr[-3000:]
    print(m.group(0))
    flagged, npatch = int(m.group(1)), int(m.group(7))
    assert flagged == npatch > 0                          # every patch went through the repair ...
    assert float(m.group(4)) < 1e-7                       # ... and comes out as accurate as the fast inversion (the probe)
    assert float(m.group(5)) <= 1e-8                      # the inverse of the PCPATCH matrix,
    assert float(m.group(6)) > 1e-6                       # which is not the inverse of the plain sub-block


def test_newton_device_and_host_assembly_agree_and_the_state_stays_on_the_device():
    """Reynolds continuation 10 -> 100 on [P3]^2-P2dg with Burman weight 5e-3 (the reference's k = 3 iters2dsv line at its
    smallest): tests/test_gpu_burman.py::test_newton_2d_device_and_host_assembly_agree (same counts, u within 1e-8) and the
    PCIe bound of tests/test_gpu_newton_state.py (at most 1 KB per Newton step in either direction)."""
    out = []
    for dev in (True, False):
        s = _solver(device_assembly=dev)
        try:
            _, i10 = s.solve(10.0)
            s.ctx.transfer_stats(reset=True)
            _, i100 = s.solve(100.0)
            h2d, d2h = s.ctx.transfer_stats()
            if dev:
                steps = i100["nonlinear_iter"]
                n_state = (s.n_u + s.n_p) * 8
                print("Newton %d + %d steps, Krylov %d + %d; %d / %d bytes across PCIe in %d steps (state %d bytes)"
                      % (i10["nonlinear_iter"], steps, i10["linear_iter"], i100["linear_iter"], h2d, d2h, steps, n_state))
                assert steps >= 2 and h2d / steps <= 1024 and d2h / steps <= 1024, (h2d, d2h, steps, n_state)
                assert n_state > 20 * 1024
            out.append((s.u.copy(), {10.0: i10, 100.0: i100}))
        finally:
            s.close()
    (ud, idev), (uh, ihost) = out
    for re in (10.0, 100.0):
        assert idev[re]["converged"] and ihost[re]["converged"], (idev[re], ihost[re])
        assert idev[re]["nonlinear_iter"] == ihost[re]["nonlinear_iter"]
        assert idev[re]["linear_iter"] == ihost[re]["linear_iter"]
    assert np.abs(ud - uh).max() < 1e-8 * np.abs(uh).max()


def test_convergence_orders_against_manufactured_solutions():
    """tests/test_gpu_mms.py::test_convergence_orders_3d_scott_vogelius_p3's margins for the 2-D pair: orders towards 4 / 3 / 3,
    the last one above 3.4 / 2.4 / 2.3; divergence below 1e-7 (the bound of test_convergence_orders_2d)."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from mms import study
    from alfi_amd.mms import convergence_orders
    hs, out = study(2, 4, [1, 2, 3], 3, "sv", [1.0], verbose=False)
    want = {"velocity": 3.4, "velocitygrad": 2.4, "pressure": 2.3}
    for name, w in want.items():
        orders = convergence_orders(out[1.0][name])
        print(name, out[1.0][name], orders)
        assert orders[-1] > w, (name, out[1.0][name], orders)
    assert max(out[1.0]["divergence"]) < 1e-7, out[1.0]["divergence"]


def _free_port():
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def test_partitioned_newton_on_two_ranks(tmp_path):
    """tests/test_gpu_dist_burman.py / test_gpu_dist_sv_state.py for [P3]^2 with Burman terms, nref 1, 2 ranks over gloo sharing
    the GPU (worker: tests/dist_gpu_sv_p3_2d_worker.py): the Newton counts of the single-GPU solver, Krylov counts within 2, u
    within 1e-7, less than 1 KB per step and rank across PCIe, no host assembly.  Every rank runs under its own time limit; the
    first rank that fails ends the test."""
    from alfi_amd.nssolver import HipNavierStokesSolver, run_solver
    from alfi_amd.problem import TwoDimLidDrivenCavityProblem
    res_list = (10, 100)
    s = HipNavierStokesSolver(TwoDimLidDrivenCavityProblem(4), 1, 3, discretisation="sv", stabilisation_type="burman",
                              stabilisation_weight=WEIGHT)
    try:
        res = run_solver(s, list(res_list))
        u_ref = s.u.copy()
    finally:
        s.close()
    port, world, limit = _free_port(), 2, 240.0
    procs = []
    try:
        for r in range(world):
            env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1",
                       MASTER_PORT=str(port), OMP_NUM_THREADS="4")
            procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "dist_gpu_sv_p3_2d_worker.py"),
                                           str(tmp_path), repr(WEIGHT)], env=env, cwd=ROOT))
        deadline = time.monotonic() + limit
        pending = list(procs)
        while pending:
            for p in list(pending):
                try:
                    code = p.wait(timeout=0.25)
                except subprocess.TimeoutExpired:
                    assert time.monotonic() < deadline, "a rank exceeded its time limit of %g s" % limit
                    continue
                assert code == 0, "a rank ended with status %d" % code
                pending.remove(p)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait(timeout=30)
    z = np.load(os.path.join(str(tmp_path), "sv_p3_2d.npz"))
    print("partitioned: Newton %s Krylov %s (single GPU %s), bytes per step and rank %s, host assemblies %s"
          % (list(z["newton"]), list(z["its"]), [(res[r]["nonlinear_iter"], res[r]["linear_iter"]) for r in res_list],
             list(z["bytes_per_step"]), list(z["host_assemblies"])))
    assert all(z["conv"]) and all(res[r]["converged"] for r in res_list)
    assert list(z["newton"]) == [res[r]["nonlinear_iter"] for r in res_list], (list(z["newton"]), res)
    assert all(abs(int(a) - res[r]["linear_iter"]) <= 2 for a, r in zip(z["its"], res_list)), (list(z["its"]), res)
    assert np.abs(z["u"] - u_ref).max() < 1e-7 * np.abs(u_ref).max()
    assert all(z["device_assembly"]) and all(z["resident"]) and all(z["partitioned"])
    assert max(z["bytes_per_step"]) < 1024, z["bytes_per_step"]
    assert list(z["host_assemblies"]) == [0] * world
