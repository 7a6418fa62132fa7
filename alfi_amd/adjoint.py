"""Adjoint solves of the Navier-Stokes Jacobian: ``NavierStokesSolver.setup_adjoint(J)`` / ``solver.solver_adjoint`` of the
reference (alfi/solver.py:520-535), every linear solve on the GPU.

After a converged ``solve(re)`` with the state z* = (u, p), the adjoint of a functional J(u, p) is

    J_F(z*)^T z_adj = -dJ/dz,      homogeneous Dirichlet conditions, the pressure nullspace as nullspace and transpose
                                   nullspace (options prefix ``ns_adj``, the same AL preconditioner and transfers).

For every pair and stabilisation built here the Jacobian is [[A, B^T], [B, 0]] with a non-symmetric velocity block A (Newton
advection, SUPG / GLS linearisations, Burman's c_F g m term) and unstabilised off-diagonal blocks (P0 / discontinuous pressure,
Burman acts on the velocity only), so J_F^T = [[A^T, B^T], [B, 0]]: only A changes.  ``AdjointSolver.solve``

1. refreshes every level's operator at z* with the parameters of the last ``solve(re)`` (nu, adv, SUPG / GLS load tables,
   GLS wind, Burman weight) -- the operators of the last Newton step belong to the previous iterate;
2. replaces them by their block transposes on the device (``hip.Level.transpose``, alfi_level_transpose: Dirichlet rows AND
   columns are identity, so the transpose keeps exactly the homogenised conditions), factors patches and coarse grid again;
3. solves with the saddle-point FGMRES of the forward solves (the Schoeberl transfers depend on (nu, gamma) only).

The next ``solve(re)`` refreshes and refactors in its first Newton step, so an adjoint solve leaves no trace in the forward
iteration.

Partitioned levels (``DistNavierStokesSolver`` with the device-side refresh): the in-place transpose is not available there --
the mirror blocks of a rank's ghost columns are other ranks' -- and not needed.  Every block of the operator is a sum over its
contributor list, and block (i, j) of A^T is the sum of the transposed MIRROR element blocks over the same list, so steps 1
and 2 become ONE refresh with ``hip.Level.set_assembly_transposed`` on (alfi_level_set_assembly_transposed): every rank forms
its own rows of A^T, no halo and no collective beyond those of the forward refresh, bitwise what refresh + transpose would
give.  Every rank forms the right-hand side from the gathered state, takes its entries (owned velocity dofs | owned pressure
rows), solves with ``DistSaddle``; ``z_adj`` is gathered onto every rank.  Still refused there: host assembly
(ALFI_DEVICE_ASSEMBLY=0 or a fallback to it).
"""
import time

import numpy as np


class LinearFunctional(object):
    """J(u, p) = g_u . u + g_p . p for fixed coefficient vectors (``g_p`` None: no pressure part)."""

    def __init__(self, g_u, g_p=None):
        self.g_u = np.asarray(g_u, dtype=np.float64)
        self.g_p = None if g_p is None else np.asarray(g_p, dtype=np.float64)

    def value(self, solver, u, p):
        v = float(self.g_u @ u)
        return v + float(self.g_p @ p) if self.g_p is not None else v

    def gradient(self, solver, u, p):
        return self.g_u, self.g_p


class LoadFunctional(LinearFunctional):
    """J(u) = int w(x) . u dx on the finest velocity space; ``w(points (N, dim)) -> (N, dim)``.  The coefficient vector is
    ``mms.load_vector`` of w, built on first use."""

    def __init__(self, w):
        self.w = w
        self.g_u, self.g_p = None, None

    def _coefficients(self, solver):
        if self.g_u is None:
            from .mms import load_vector
            self.g_u = load_vector(solver.levels[-1].V, self.w)
        return self.g_u

    def value(self, solver, u, p):
        return float(self._coefficients(solver) @ u)

    def gradient(self, solver, u, p):
        return self._coefficients(solver), None


def adjoint_rhs(g_u, g_p, bc_dofs, n_p, vol=None):
    """-(g_u, g_p) as the right-hand side of J_F^T z_adj = -dJ/dz: the Dirichlet velocity entries zeroed (``homogenize(bcs)``:
    the forward state's Dirichlet values do not vary) and, with a pressure nullspace (``vol``: the weights of the pressure
    integral), the pressure part replaced by P^T g_p, P = I - 1 vol^T / |domain| -- the transpose of the zero-integral
    normalisation the forward solve applies to p.  Its entries sum to zero, so the right-hand side lies in the range of J_F^T
    (orthogonal to (0, 1_p), since B^T 1 = 0); with equal cell volumes this is the removal of the plain mean."""
    rhs_u = -np.array(g_u, dtype=np.float64)
    rhs_u[np.asarray(bc_dofs, dtype=np.int64)] = 0.0
    rhs_p = np.zeros(n_p) if g_p is None else -np.array(g_p, dtype=np.float64)
    if vol is not None:
        vol = np.asarray(vol, dtype=np.float64)
        rhs_p -= vol * (rhs_p.sum() / vol.sum())
    return np.concatenate([rhs_u, rhs_p])


def as_functionals(J):
    """(list of functionals, is_list): a list or tuple of functionals is a block of adjoint right-hand sides, anything else ONE
    functional -- and then every return type is the single functional's."""
    if isinstance(J, (list, tuple)):
        if len(J) == 0:
            raise ValueError("an empty list of functionals")
        return list(J), True
    return [J], False


def adjoint_rhs_block(gradients, bc_dofs, n_p, vol=None):
    """(n_u + n_p, K) matrix whose column i is ``adjoint_rhs`` of ``gradients[i] = (g_u, g_p)``: built column by column."""
    return np.stack([adjoint_rhs(g_u, g_p, bc_dofs, n_p, vol) for g_u, g_p in gradients], axis=1)


class AdjointSolver(object):
    """``solver.solver_adjoint``: ``solve(rtol=None, atol=None)`` writes ``solver.z_adj = (lam_u, lam_p)`` (host arrays) for the
    functional given to ``setup_adjoint`` and returns an info dict.  Given a LIST (or tuple) of K functionals it refreshes,
    transposes and factors ONCE, solves the K systems with one ``Saddle.solve_block`` (the patch factors streamed once for up
    to four of them), writes ``solver.z_adj = [(lam_u, lam_p), ...]`` and returns ``linear_iter``, ``residual_norm``,
    ``rhs_norm`` and ``converged`` as lists with one entry per functional; the times stay single numbers."""

    def __init__(self, solver, J):
        self.solver, self.J = solver, J
        self.functionals, self.is_list = as_functionals(J)

    def _operators(self, adv):
        """Transposed Jacobian blocks of z* on every level, factored.  Returns (refresh, transpose, factor) seconds."""
        s = self.solver
        if s._partitioned:
            return self._operators_partitioned(adv)
        mgl = s.hmg.mg.levels
        saved = dict(s.timings)
        t0 = time.time()
        if s.device_assembly:
            if not (s._device_newer or s._device_current):
                s._push_state()
                s._device_current = True
            s._refresh_device(None, adv)
        else:
            # host assembly: the values of z* are uploaded (and, on this path, factored once for the forward operator)
            s._rediscretise(s.u.copy(), adv)
            s.ctx.sync()
        t1 = time.time()
        for dl in (mgl[-1:] if getattr(s, "allu", False) else mgl):     # allu factors the finest operator alone
            dl.transpose()
        s.ctx.sync()
        t2 = time.time()
        s._factor_levels()
        t3 = time.time()
        s.timings.clear()
        s.timings.update(saved)            # the forward solve's accounting stays the forward solve's
        return t1 - t0, t2 - t1, t3 - t2

    def _operators_partitioned(self, adv):
        """Partitioned levels: every rank refreshes ITS rows of the transposed operators on the device -- the transposed
        refresh about z*, through the state exchange or (``device_state=False``) the uploaded states --, then the factors."""
        s = self.solver
        saved = dict(s.timings)
        t0 = time.time()
        levels = [dl for dl, _, _ in s._device_levels()]
        try:
            with s._on_stream():
                for dl in levels:
                    dl.set_assembly_transposed(True)
            if s._device_state_resident():
                if not (s._device_newer or s._device_current):
                    s._push_state()
                    s._device_current = True
                s._refresh_device(None, adv)
            else:                           # the replicated host state, uploaded into every level's state vector
                s._refresh_device(s.u.copy(), adv)
        finally:
            with s._on_stream():
                for dl in levels:
                    dl.set_assembly_transposed(False)
        t1 = time.time()
        s._factor_levels()
        t2 = time.time()
        s.timings.clear()
        s.timings.update(saved)
        return t1 - t0, 0.0, t2 - t1

    def _solve_partitioned(self, t0, times, rtol, atol):
        """Right-hand sides from the gathered state on every rank (``u`` / ``p`` gather collectively), the rank's entries
        solved with DistSaddle (a list: its columns one after the other), the adjoints gathered onto every rank."""
        s = self.solver
        sad = s.saddle
        t_ref, t_tr, t_fac = times
        u, p = s.u, s.p
        rhs = adjoint_rhs_block([J.gradient(s, u, p) for J in self.functionals], s.levels[-1].bc_dofs, s.n_p,
                                s.vol if s.nullspace else None)
        rtol = s.rtol if rtol is None else float(rtol)
        atol = s.atol if atol is None else float(atol)
        max_it = s.params["ksp_max_it"]
        loc = np.ascontiguousarray(np.concatenate([rhs[:s.n_u][s._own_dofs], rhs[s.n_u:][np.asarray(sad.cells)]]))
        t_s = time.time()
        # (alfi_saddle_solve_block takes serial saddles only: the columns of a list are solved one after the other with the ONE
        # set of factors -- block right-hand sides on partitioned levels are looped)
        cols = [sad.solve(np.ascontiguousarray(loc[:, c]), rtol, atol, max_it, 30) for c in range(loc.shape[1])]
        x = np.stack([c[0] for c in cols], axis=1)
        its, rn = [c[1] for c in cols], [c[2] for c in cols]
        lam = np.zeros((s.n_u + s.n_p, rhs.shape[1]))
        for dofs, cells, xu, xp in s.dmg.comm.all_gather_object((s._own_dofs, sad.cells, x[:sad.n_own], x[sad.n_own:sad.n])):
            lam[dofs] = xu
            lam[s.n_u + np.asarray(cells, dtype=np.int64)] = xp
        t_solve = time.time() - t_s
        z = []
        for c in range(rhs.shape[1]):
            lam_u, lam_p = lam[:s.n_u, c].copy(), lam[s.n_u:, c].copy()
            if s.nullspace:              # zero integral, as the forward solve shifts p
                lam_p -= (s.vol @ lam_p) / s.area
            z.append((lam_u, lam_p))
        bnorm = [float(np.linalg.norm(rhs[:, c])) for c in range(rhs.shape[1])]
        conv = [bool(i < max_it or r <= max(rtol * b, atol)) for i, r, b in zip(its, rn, bnorm)]
        if not self.is_list:
            z, its, rn, bnorm, conv = z[0], its[0], rn[0], bnorm[0], conv[0]
        s.z_adj = z
        return {"linear_iter": its, "time": (time.time() - t0) / 60.0, "residual_norm": rn, "rhs_norm": bnorm, "converged": conv,
                "refresh_s": t_ref, "transpose_s": t_tr, "factor_s": t_fac, "solve_s": t_solve}

    def solve(self, rtol=None, atol=None):
        s = self.solver
        if getattr(s, "_last_solve", None) is None:
            raise RuntimeError("adjoint solve before any solve(re): the adjoint is taken about a converged state")
        _, adv = s._last_solve
        t0 = time.time()
        t_ref, t_tr, t_fac = self._operators(adv)
        if s._partitioned:
            return self._solve_partitioned(t0, (t_ref, t_tr, t_fac), rtol, atol)
        if self.is_list:
            return self._solve_block(t0, (t_ref, t_tr, t_fac), rtol, atol)
        u, p = s.u, s.p
        g_u, g_p = self.J.gradient(s, u, p)
        rhs = adjoint_rhs(g_u, g_p, s.levels[-1].bc_dofs, s.n_p, s.vol if s.nullspace else None)
        rtol = s.rtol if rtol is None else float(rtol)
        atol = s.atol if atol is None else float(atol)
        t_s = time.time()
        db, dx = s.ctx.vec(rhs), s.ctx.vec(s.n_u + s.n_p)
        max_it = s.params["ksp_max_it"]
        its, rn = s.saddle.solve(db, dx, rtol, atol, max_it, 30)
        lam = dx.get()
        t_solve = time.time() - t_s
        lam_u, lam_p = lam[:s.n_u].copy(), lam[s.n_u:].copy()
        if s.nullspace:                  # zero integral, as the forward solve shifts p (solver.py:273-277)
            lam_p -= (s.vol @ lam_p) / s.area
        s.z_adj = (lam_u, lam_p)
        bnorm = float(np.linalg.norm(rhs))
        return {"linear_iter": its, "time": (time.time() - t0) / 60.0, "residual_norm": rn, "rhs_norm": bnorm,
                # (FGMRES stops on its recurrence residual; the true one, reported, may differ from it by rounding)
                "converged": bool(its < max_it or rn <= max(rtol * bnorm, atol)), "refresh_s": t_ref, "transpose_s": t_tr,
                "factor_s": t_fac, "solve_s": t_solve}


    def _solve_block(self, t0, times, rtol, atol):
        """The K functionals of a list after ONE ``_operators`` pass: right-hand sides column by column, one block solve."""
        s = self.solver
        t_ref, t_tr, t_fac = times
        rhs = adjoint_rhs_block([J.gradient(s, s.u, s.p) for J in self.functionals], s.levels[-1].bc_dofs, s.n_p,
                                s.vol if s.nullspace else None)
        rtol = s.rtol if rtol is None else float(rtol)
        atol = s.atol if atol is None else float(atol)
        t_s = time.time()
        dB, dX = s.ctx.mat(rhs), s.ctx.mat(s.n_u + s.n_p, rhs.shape[1])
        max_it = s.params["ksp_max_it"]
        its, rn = s.saddle.solve_block(dB, dX, rtol, atol, max_it, 30)
        lam = dX.get()
        t_solve = time.time() - t_s
        s.z_adj = []
        for c in range(rhs.shape[1]):
            lam_u, lam_p = lam[:s.n_u, c].copy(), lam[s.n_u:, c].copy()
            if s.nullspace:              # zero integral per column, as the forward solve shifts p
                lam_p -= (s.vol @ lam_p) / s.area
            s.z_adj.append((lam_u, lam_p))
        bnorm = [float(np.linalg.norm(rhs[:, c])) for c in range(rhs.shape[1])]
        return {"linear_iter": its, "time": (time.time() - t0) / 60.0, "residual_norm": rn, "rhs_norm": bnorm,
                "converged": [bool(i < max_it or r <= max(rtol * b, atol)) for i, r, b in zip(its, rn, bnorm)],
                "refresh_s": t_ref, "transpose_s": t_tr, "factor_s": t_fac, "solve_s": t_solve}


def setup_adjoint(solver, J):
    """``solver.setup_adjoint(J)``: keep the functional -- or the list of functionals -- and create ``solver.solver_adjoint``."""
    if solver._partitioned and not (getattr(solver, "_asm_ready", False) and getattr(solver, "device_assembly", False)):
        # (read before any collective: every rank reaches the same verdict, the fallback to host assembly is agreed on)
        raise NotImplementedError("adjoint solves on partitioned levels need the device-side operator refresh (the transposed "
                                  "refresh, alfi_level_set_assembly_transposed): with host assembly the mirror blocks of a "
                                  "rank's ghost columns belong to other ranks")
    solver.J_adj = J
    solver.solver_adjoint = AdjointSolver(solver, J)
    return solver.solver_adjoint


def gradient(solver, dF_dm, dJ_dm=0.0, index=None):
    """dJ/dm = dJ/dm|_z + z_adj . dF/dm for a parameter m the residual depends on, with the adjoint of the last
    ``solver_adjoint.solve()``; ``dF_dm``: (dF_u/dm, dF_p/dm) or the concatenated vector, Dirichlet rows zeroed as F's.
    ``index``: which functional of a list (``solver.z_adj`` is then a list of adjoints); None for a single functional."""
    if isinstance(solver.z_adj, list):
        if index is None:
            raise ValueError("solver.z_adj holds %d adjoints: say which one (index=)" % len(solver.z_adj))
        lam_u, lam_p = solver.z_adj[index]
    else:
        if index is not None:
            raise ValueError("solver.z_adj holds one adjoint: no index")
        lam_u, lam_p = solver.z_adj
    v = np.concatenate(dF_dm) if isinstance(dF_dm, tuple) else np.asarray(dF_dm)
    return float(dJ_dm) + float(lam_u @ v[:len(lam_u)] + lam_p @ v[len(lam_u):])


__all__ = ["LinearFunctional", "LoadFunctional", "AdjointSolver", "adjoint_rhs", "adjoint_rhs_block", "as_functionals", "setup_adjoint",
           "gradient"]
