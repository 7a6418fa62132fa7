"""The solve loop around the hot path: Newton on the stationary Navier-Stokes equations with Reynolds continuation, as
``alfi.solver.NavierStokesSolver.solve`` / ``alfi.driver.run_solver`` organise it (alfi/solver.py:257-300,
alfi/driver.py:95-128), every linear solve on the GPU.

Per Newton step (``snes_type newtonls``, basic line search, solver.py:463-472):

1. host: rediscretise the velocity block about the current velocity on every level -- the state reaches the coarse
   levels by ``inject`` (solver.py:595; here the index map of ``fespace.injection_map``) -- and hand the new values to
   the device hierarchy (``HipPatchPC.update`` -> re-gather and re-invert every patch, new coarse inverse);
2. host: nonlinear residual F(u, p) of solver.py:565-568 with the [P_k(+FB)]^d - P0 pair,
   F_u = A0 u + 1/2 N(u) u + B^T p,  F_p = B u   (N(u) v = (u.grad) v + (v.grad) u, so N(u) u = 2 (u.grad) u);
3. device: J d = -F by ``alfi_saddle_solve`` (FGMRES + fieldsplit Schur full, PCMG full cycles, DGMassInv).

``solver_type`` (alfi/solver.py:346-422): "almg" (the default, fieldsplit_0 = PCMG) or "allu" (fieldsplit_0 = an exact solve
with the library's multifrontal factors of the finest operator: the ideal augmented-Lagrangian check, examples/Makefile
``idealal``).  With allu a Newton step refreshes and factors the finest operator only -- no patches, no coarse grid.

The generator plays Firedrake's role (assembly, setup time); the arithmetic of the solves is libalfi_hip.so's.
"""
import contextlib
import time
import warnings

import numpy as np

from . import _hostlib, env, hip
from .problem import BSR, build_hierarchy, build_pressure_coupling
from .solver import HipMG, mg_levels_solver, fieldsplit_0_mg, fieldsplit_0_lu, outer_solver

SOLVER_TYPES = ("almg", "allu", "alamg", "lu", "simple", "lsc")     # alfi/driver.py:18 (--solver-type)


def check_solver_type(solver_type, partitioned=False):
    """The reference's solver types: almg and allu are built; the others raise NotImplementedError with the reason, an unknown
    name ValueError.  Host-only: runs before any device work."""
    if solver_type not in SOLVER_TYPES:
        raise ValueError("unknown solver_type %r (one of %s)" % (solver_type, ", ".join(SOLVER_TYPES)))
    if solver_type == "lu":
        raise NotImplementedError("solver_type 'lu' (a monolithic LU of the saddle-point Jacobian) needs pivoting on the zero "
                                  "pressure block; the multifrontal fronts are factored without pivoting")
    if solver_type in ("simple", "lsc", "alamg"):
        raise NotImplementedError("solver_type %r needs an algebraic multigrid (hypre in the reference), which is not built"
                                  % solver_type)
    if solver_type == "allu" and partitioned:
        raise NotImplementedError("solver_type 'allu' on partitioned levels: the multifrontal factorisation is single-rank")


def _assemble(L, nu, gamma, adv, wind, with_bc, full_div=False):
    """full_div: the Scott-Vogelius grad-div term gamma (div u, div v) (solver.py:616) instead of the cell-averaged one."""
    V = L.V
    g, vol = V.mesh.cell_geometry()
    tens = V.element.reference_tensors()
    A = _hostlib.assemble_bsr(V.cell_nodes, g, vol, tens, V.dim, L.A.rowptr, L.A.colidx, nu=nu,
                              gamma=0.0 if full_div else gamma, gamma_full=gamma if full_div else 0.0, adv=adv,
                              wind=wind if adv else None)
    if with_bc:
        _hostlib.apply_bc_bsr(V.num_nodes, V.dim, L.A.rowptr, L.A.colidx, A, np.repeat(V.bc_node_mask, V.dim))
    return A


class HipNavierStokesSolver(object):
    """``solve(re)`` mirrors NavierStokesSolver.solve (solver.py:257-300): returns (z, info_dict) with the reference's
    keys Re, nu, linear_iter, nonlinear_iter, time."""

    def __init__(self, problem, nref, k, gamma=1e4, smoothing=None, restriction=False, ctx=None, verbose=False,
                 snes_rtol=None, snes_atol=None, snes_stol=1e-6, snes_max_it=20, discretisation="pkp0", stabilisation_type=None,
                 stabilisation_weight=None, supg_magic=9.0, device_assembly=None, solver_type="almg", direct_max_bytes=0,
                 patch_factor_dtype=None, macro_factor_dtype=None):
        """discretisation: "pkp0" ([P_k(+FB)]^d - P0 on the uniform hierarchy, ConstantPressureSolver solver.py:561-602) or
        "sv" ([P_k]^d - P_{k-1}^dg on the barycentric hierarchy with macro-star patches, ScottVogeliusSolver :604-662).
        stabilisation_type: None / "none", "supg" or "gls" (P0-pressure pairs; GLS's wind is the velocity at the start of each
        ``solve``, solver.py:199, 205, 215) or "burman" (the Scott-Vogelius pair: interior-penalty
        term of stabilisation.py:139-162 on facet-coupled levels, alfi_amd.burman; on partitioned levels in
        alfi_amd.dist_nssolver.DistNavierStokesSolver, every rank the facets of its cells).
        device_assembly: refresh the level operators of every Newton step ON THE DEVICE (alfi_level_assemble: what
        PatchPC.update does inside PCPATCH, solver.py:320, 325) instead of rediscretising on the host and re-uploading;
        default: on (viscous, grad-div, advection and SUPG terms), unless ALFI_DEVICE_ASSEMBLY=0.
        solver_type: "almg" (fieldsplit_0 = PCMG full cycle, the default) or "allu" (fieldsplit_0 = exact solve with multifrontal
        factors of the finest operator, re-factored every Newton step; ``smoothing`` / ``restriction`` are then accepted and
        ignored, as on the reference's idealal lines); "lu", "simple", "lsc", "alamg": NotImplementedError.
        direct_max_bytes: allu only -- cap on the factors + front storage in bytes (0: the free device memory).
        patch_factor_dtype: None, or "f32": the smoothed levels store their dense patch inverses in single precision where that
        form exists (hip.ask_patch_storage); every refactorisation of a Newton step converts again.
        macro_factor_dtype: None, or "f32": the same for macro stars and Burman levels (hip.ask_macro_patch_storage; levels that
        store condensed factors on the generator's groups keep them in FP64).  One of the two keywords at most (ValueError)."""
        hip.check_factor_dtypes(patch_factor_dtype, macro_factor_dtype)
        self._patch_factor_dtype, self._macro_factor_dtype = patch_factor_dtype, macro_factor_dtype
        check_solver_type(solver_type, self._partitioned)
        self.solver_type = solver_type
        self.allu = solver_type == "allu"
        self.direct_max_bytes = int(direct_max_bytes)
        self.problem, self.gamma, self.verbose = problem, float(gamma), verbose
        if device_assembly is None:
            device_assembly = env.device_assembly()
        self.device_assembly = bool(device_assembly)
        self.timings = {"assemble_s": 0.0, "factor_s": 0.0, "residual_s": 0.0, "solve_s": 0.0, "newton_steps": 0}
        self._ctx_arg = ctx
        dim = problem.dim
        self.sv = discretisation == "sv"
        # stabilisation (solver.py:56-58, 66-68, 204-234): SUPG with the Shakib-Hughes-Johan coefficient (supg_method
        # "shakib", the default), default weight 0.1 in 3-D and 1 in 2-D (stabilisation.py:52-54), supg_magic 9
        if stabilisation_type in ("none", None):
            stabilisation_type = None
        if stabilisation_type not in (None, "supg", "gls", "burman"):
            raise NotImplementedError("stabilisation type %r (built: supg and gls for the P0-pressure pairs, burman for the "
                                      "Scott-Vogelius pair)" % stabilisation_type)
        if stabilisation_type in ("supg", "gls") and self.sv:
            raise NotImplementedError("%s with a discontinuous P_k pressure couples grad p into the momentum block"
                                      % stabilisation_type)
        if stabilisation_type == "gls" and self._partitioned:
            raise NotImplementedError("gls on partitioned levels: the wind of every rank's cells would need its own exchange")
        if stabilisation_type == "burman" and not self.sv:
            raise NotImplementedError("burman is built for the Scott-Vogelius pair (discretisation='sv') only")
        self.supg = stabilisation_type == "supg"
        # GLS (solver.py:204-234): the SUPG coefficient, weights and quadrature, the test side L_w v about the wind w = z_last
        self.gls = stabilisation_type == "gls"
        # Burman interior penalty (solver.py:226-228, stabilisation.py:139-162): weight 3e-3 unless given (the reference's
        # SV run lines pass 5e-3)
        self.burman = stabilisation_type == "burman"
        if self.burman:
            from .burman import DEFAULT_WEIGHT
            self.burman_weight = float(stabilisation_weight) if stabilisation_weight is not None else DEFAULT_WEIGHT
        self.supg_weight = float(stabilisation_weight) if stabilisation_weight is not None else (0.1 if dim == 3 else 1.0)
        self.supg_magic = float(supg_magic)
        self.char_L, self.char_U = problem.char_length(), problem.char_velocity()
        self.nullspace = bool(problem.has_nullspace())
        # hierarchy and device objects are created once (Stokes operator); values are replaced per Newton step
        self._values_on_device = False
        if self.sv:
            from .sv import build_sv_hierarchy, build_sv_pressure_coupling
            self.levels, self.transfers = build_sv_hierarchy(problem, nref, k, Re=0.0, gamma=gamma, facet_coupling=self.burman)
        else:
            # with the device-side refresh nobody reads a host copy of the operators: the generator then delivers the sparsity
            # only and the first (Stokes) operator is formed on the device as well (no host assembly, no 8 GB upload at config 4)
            self._values_on_device = self.device_assembly
            self.levels, self.transfers = build_hierarchy(problem, nref, k, Re=0.0, gamma=gamma, lazy=self._lazy_generation(),
                                                          operator_values=not self._values_on_device)
        if self.sv:      # patch = macro with the problem's relaxation direction (solver.py:339-342), sparse-LU patch options
            from .solver import configure_patch_solver_sv
            mgl = configure_patch_solver_sv(mg_levels_solver(dim, patch="macro", smoothing=smoothing,
                                                             relaxation_direction=problem.relaxation_direction()), dim)
        else:
            mgl = mg_levels_solver(dim, smoothing=smoothing)
        # (allu: the multigrid hierarchy is still built -- its levels and transfers carry the refresh and the state injection)
        self._fieldsplit_0_mg = fieldsplit_0_mg(mgl)
        self.params = outer_solver(dim, fieldsplit_0_lu() if self.allu else self._fieldsplit_0_mg)
        L = self.levels[-1]
        self.nu = self.char_L * self.char_U
        self.Minv = None
        if self.sv:
            # B with the Dirichlet columns zeroed (the Jacobian's) and with all columns (the residual's), one pass
            self.B, self.B_raw, M, self.Minv = build_sv_pressure_coupling(L, both=True)
            self.vol = np.asarray(M.sum(axis=1)).ravel()                    # int psi_j: weights of the pressure integral
        else:
            # Dirichlet columns zeroed: the Jacobian's B; all columns: the residual's B
            self.B, self.B_raw, self.vol = build_pressure_coupling(L, both=True)
        self._create_device(restriction)
        self._asm_ready = False
        self._start_device_assembly()
        self.rtol, self.atol = self.params["ksp_rtol"], self.params["ksp_atol"]
        tol2, tol3 = (1e-9, 1e-8), (1e-8, 1e-8)                            # snes_rtol / snes_atol, solver.py:484-499
        self.snes_rtol = snes_rtol if snes_rtol is not None else (tol2 if dim == 2 else tol3)[0]
        self.snes_atol = snes_atol if snes_atol is not None else (tol2 if dim == 2 else tol3)[1]
        self.snes_stol = snes_stol                                          # solver.py:490, 498
        self.snes_max_it = snes_max_it
        self.n_u, self.n_p = L.n, self.B.shape[0]
        # state z = (u, p): zero with the Dirichlet values imposed (what Firedrake does to the initial guess).  With the
        # device-side refresh the state LIVES on the device (``_dz``); ``u`` / ``p`` fetch it when somebody asks.
        self._host_u = np.zeros(self.n_u)
        bc_nodes = L.V.bc_nodes
        self._host_u.reshape(-1, dim)[bc_nodes] = problem.driver(L.V.node_coords[bc_nodes])
        self._host_p = np.zeros(self.n_p)
        self._device_newer = False          # the device copy of the state is ahead of the host arrays
        self._device_current = False        # the device copy equals the host arrays
        self._load = None
        self._fq = None                     # per level: the body force at the SUPG / GLS points (supg_load), or None
        self._host_winds = None             # GLS on the host path: the wind on every level
        self._last_solve = None             # (re, adv) of the last solve: the adjoint's operators use the same parameters
        self.area = float(self.vol.sum())

    # -- the state: host arrays on request, resident on the device during the solves -------------------------------------
    def _fetch_state(self):
        if self._device_newer:
            z = self._dz.get()
            self._host_u, self._host_p = z[:self.n_u].copy(), z[self.n_u:].copy()
            self._device_newer, self._device_current = False, True

    @property
    def u(self):
        self._fetch_state()
        return self._host_u

    @u.setter
    def u(self, value):
        self._fetch_state()
        self._host_u = np.asarray(value, dtype=np.float64)
        self._device_current = False

    @property
    def p(self):
        self._fetch_state()
        return self._host_p

    @p.setter
    def p(self, value):
        self._fetch_state()
        self._host_p = np.asarray(value, dtype=np.float64)
        self._device_current = False

    # -- device side (overridden by alfi_amd.dist_nssolver.DistNavierStokesSolver for partitioned levels) ----------------
    _partitioned = False                    # whether the levels are partitioned over ranks

    def _any_rank(self, flag):
        """True if ``flag`` holds on any rank (one rank here)."""
        return bool(flag)

    def _on_stream(self):
        """The context the device calls are made in (partitioned: the library's stream current for torch)."""
        return contextlib.nullcontext()

    @contextlib.contextmanager
    def _timed(self, key):
        """The wall time of the block is added to ``timings[key]``."""
        t = time.time()
        yield
        self.timings[key] += time.time() - t

    def _lazy_generation(self):
        """Operators and transfers as recipes that assemble the rows somebody asks for (alfi_amd.lazy) instead of global
        values: for the partitioned solver, whose ranks only ever need their own rows."""
        return False

    def _create_device(self, restriction):
        self.ctx = self._ctx_arg or hip.Context(0)
        self.hmg = HipMG(self.ctx, self.levels, self.transfers, self._fieldsplit_0_mg, restriction=restriction,
                         patch_factor_dtype=self._patch_factor_dtype, macro_factor_dtype=self._macro_factor_dtype)
        self.saddle = hip.Saddle(self.hmg.mg, self.B, None if self.sv else self.vol, self.nu, self.gamma,
                                 remove_constant_nullspace=self.nullspace, mass_inv=self.Minv)
        self._ksp, self._device_transfers = self.saddle, list(zip(self.transfers, self.hmg.mg.transfers))
        self._own_dofs = self._own_cells = slice(None)
        self._n_own, self._np_own = self.levels[-1].n, self.B.shape[0]
        if self.allu:
            self.saddle.set_velocity_solver("direct")
        if getattr(self, "burman", False):   # PCPATCH's facet rule in the patch matrices of the Burman levels
            from .burman import patch_facet_corrections
            for L, obj in zip(self.levels, self.hmg.pc_objs):
                if obj is not None:
                    obj.level.set_patch_facet_correction(L.facets.nf, *patch_facet_corrections(L.V, L.facets, obj.patch_ptr,
                                                                                               obj.patch_dofs))

    def _push_operators(self):
        """New operator values on every level: re-gather and re-invert the patches, new coarse inverse (allu: the finest
        operator's values and its direct factorisation only)."""
        if self.allu:
            self.hmg.mg.levels[-1].update_values(self.levels[-1].A.vals)
            self._factor_direct()
            return
        self.hmg.update(self.levels)
        self.hmg.mg.levels[0].update_values(self.levels[0].A.vals)
        self.hmg.mg.levels[0].coarse_factor_auto()

    # -- operator refresh on the device ---------------------------------------------------------------------------------------
    def _start_device_assembly(self):
        """The device-side refresh set up -- first the rank-local part, then the exchange of the distributed state -- or, if any
        rank fails at either, host assembly on ALL ranks; then the first (Stokes) operators where the generator left them out.
        Partitioned: every rank, failing or not, meets the others in ``_any_rank`` after each phase and nowhere else before it
        (the phases' own collectives start only once all ranks have passed the agreement before them) -- one rank on the host
        path and the others on the device path would call different collectives."""
        phases = (self._setup_device_assembly, self._setup_state_exchange) if self.device_assembly else ()
        for phase in phases:
            failure = None
            try:
                phase()
            except hip.AlfiHipError as e:
                failure = e
            if self._any_rank(failure is not None):
                # (e.g. ALFI_SPMV=legacy: the refresh writes the lane-major operator layout): fall back, say so
                warnings.warn("device-side operator refresh not available (%s): the operators of every Newton step are "
                              "assembled on the host" % (failure if failure is not None else "another rank failed to set it up",))
                self.device_assembly = False
                break
        if self._values_on_device:
            if self.device_assembly:
                self._first_operators_on_device()
            else:                           # the refresh could not be set up after all: the host assembler's Stokes operators
                for Lv in self.levels:
                    Lv.A = BSR(Lv.A.nbrows, Lv.A.nbcols, Lv.bs, Lv.A.rowptr, Lv.A.colidx,
                               _assemble(Lv, self.nu, self.gamma, 0.0, None, True, full_div=self.sv))
                self._values_on_device = False
                self._push_operators()

    def _setup_device_assembly(self):
        """Once: the cells, the reference tensors of the element and the contributor lists of every level go to the device
        (alfi_level_set_assembly: every term of the operator is formed there, cell by cell); per-level state vectors for the
        injected field."""
        self._dstate = []
        for L, dl in zip(self.levels, self.hmg.mg.levels):
            if self.burman:
                dl.set_facet_blocks(True)
            dl.set_assembly(L.V, L.A.rowptr, L.A.colidx, full_div=self.sv)
            if self.supg or self.gls:
                dl.set_supg(L.V)
            if self.burman:
                dl.set_burman(L.facets, L.A.rowptr, L.A.colidx)
            self._dstate.append(self.ctx.vec(L.n))
        # GLS: the wind on every level, filled at the start of each solve (the finest from the resident state, then injected)
        self._dwind = [self.ctx.vec(L.n) for L in self.levels] if self.gls else None
        # the Newton state z = (u | p), the residual F and the update live on the device; the finest level's state vector IS
        # the velocity part of z
        n = self.levels[-1].n + self.B_raw.shape[0]
        self._dz, self._dF, self._dd = self.ctx.vec(n), self.ctx.vec(n), self.ctx.vec(n)
        self._dstate[-1] = hip.view(self._dz, 0, self.levels[-1].n)
        self._dres = self.ctx.vec(self.levels[-1].n)
        # the residual's divergence products on the device too (B with ALL columns; the Jacobian's B lives in the saddle
        # solver): at config-4 size the two host products were 0.13 s of a 0.2 s residual
        self._dB = hip.Csr(self.ctx, self.B_raw)
        self._dBT = hip.Csr(self.ctx, self.B_raw.T.tocsr())
        self._dp, self._dFp = self.ctx.vec(self.B_raw.shape[0]), self.ctx.vec(self.B_raw.shape[0])
        self._asm_ready = True

    def _setup_state_exchange(self):
        """Second phase of the set-up: what needs the other ranks (nothing on one GPU)."""

    def _device_levels(self):
        """(device level, its state vector, its GLS wind or None) of every level this rank assembles, coarsest first."""
        return list(zip(self.hmg.mg.levels, self._dstate, self._dwind or [None] * len(self.levels)))

    def _assemble_level(self, dl, st, wind, adv):
        """The operator of one device level formed about the state ``st`` (``wind``: GLS's)."""
        if adv and self.supg:     # A = nu K + gamma D + N(w) + the linearised SUPG term, THEN the boundary conditions
            dl.assemble_supg(self.nu, self.gamma, adv, st, self.supg_weight, self.supg_magic, True)
        elif adv and self.gls:    # ... + the linearised GLS term with the solve's wind
            dl.assemble_gls(self.nu, self.gamma, adv, st, wind, self.supg_weight, self.supg_magic, True)
        elif adv and self.burman:  # ... + adv * the linearised Burman term (a facet pass), then the boundary conditions
            dl.assemble_burman(self.nu, self.gamma, adv, st, self.burman_weight, True)
        else:
            dl.assemble(self.nu, self.gamma, adv, st if adv else None, True)

    def _first_operators_on_device(self):
        """The Stokes operators the hierarchy is created with (what build_hierarchy(Re=0) assembles on the host otherwise),
        formed on the device; patches and coarse grid factored."""
        with self._on_stream():
            for dl, _, _ in self._device_levels():
                self._assemble_level(dl, None, None, 0.0)
            self.ctx.sync()
        if not self.allu:                   # (allu: the first Newton step factors the operator it solves with)
            self._factor_levels()

    def _device_states(self, u):
        """Current velocity on every level, on the device: the finest is the velocity part of the resident state (``u`` given:
        uploaded into it first), the coarser ones by alfi_inject (solver.py:595) -- an index map on the nested hierarchies, the
        point-evaluation matrix sv.bary_injection on the barycentric ones (the third entry of the reference's transfer triple,
        solver.py:645-652)."""
        if u is not None:
            self._fetch_state()
            self._dstate[-1].set(u)
            self._device_current = False
        for l in range(len(self.levels) - 1, 0, -1):
            self.hmg.mg.transfers[l - 1].inject(self._dstate[l], self._dstate[l - 1])

    def _rediscretise_device(self, u, adv):
        with self._timed("assemble_s"):
            self._refresh_device(u, adv)
        with self._timed("factor_s"):
            self._factor_levels()

    def _refresh_device(self, u, adv):
        """Every level's operator formed on the device about the current state (the first half of a Newton step's refresh);
        allu solves with the finest operator alone."""
        with self._on_stream():
            self._device_states(u)
            for dl, st, wind in self._device_levels()[-1 if self.allu else 0:]:
                self._assemble_level(dl, st, wind, adv)
            self.ctx.sync()

    def _factor_levels(self):
        """Patches of every level and the coarse grid factored from the operator values the device holds (allu: the direct
        factorisation of the finest operator instead)."""
        if self.allu:
            return self._factor_direct()
        mgl = self.hmg.mg.levels
        for L, dl in zip(self.levels, mgl):
            L.nu = self.nu
            if L.level > 0:
                dl.factor_with_fallback()
        mgl[0].coarse_factor_auto()
        self.ctx.sync()

    def _factor_direct(self):
        """allu: numeric factorisation of the finest operator the device holds (plan of the first call reused); the probe
        residual of the new factors is kept in ``direct_residual``."""
        for L in self.levels:
            L.nu = self.nu
        self.direct_residual = self.saddle.factor_velocity(max_bytes=self.direct_max_bytes)
        self.ctx.sync()

    def _residual_device(self, u, p, adv):
        """F_u = (nu K + gamma D) u + 1/2 N(u) u + B^T p - f: one matrix-free product, cell by cell, with HALF the advection
        term and without boundary conditions (N(u) u = 2 (u . grad) u)."""
        self._fetch_state()                                                # (the host arrays keep what the device held)
        self._dz.set(np.concatenate([u, p]))
        self._device_current = False
        self._residual_on_device(adv)
        F = self._dF.get()
        return F[:self.n_u], F[self.n_u:]

    def _velocity_residual(self, fin, st, wind, adv, out):
        """out = (nu K + gamma D + 1/2 N(u)) u (+ the stabilisation's residual) for the finest level's state ``st``."""
        fin.assemble_mult(self.nu, self.gamma, 0.5 * adv, st if adv else None, st, out)
        if adv and self.supg:         # + the SUPG residual, gathered on the device into the same vector
            fin.supg(self.nu, self.supg_weight, self.supg_magic, st, False, out)
        if adv and self.gls:          # + the GLS residual with the solve's wind
            fin.gls(self.nu, self.supg_weight, self.supg_magic, st, wind, False, out)
        if adv and self.burman:       # + advect * the Burman residual (solver.py:233-234), facet pass + node gather
            fin.burman(adv * self.burman_weight, st, False, out)

    def _momentum_residual(self, fin, st, wind, dp, adv, Fu):
        """Fu = the velocity terms + B^T p (partitioned: the rank's share of B^T p goes through the halo onto the owners)."""
        self._velocity_residual(fin, st, wind, adv, Fu)
        self._dBT.mult(dp, Fu, mode=2)                                    # F_u += B^T p

    def _residual_on_device(self, adv):
        """F(z) for the state resident in ``_dz`` into ``_dF`` = (F_u | F_p), every rank its owned entries; nothing crosses to
        the host."""
        fin, st, wind = self._device_levels()[-1]
        n_u, n_p = self._n_own, max(self._np_own, 1)
        Fu = hip.view(self._dF, 0, n_u)
        with self._on_stream():
            self._momentum_residual(fin, st, wind, hip.view(self._dz, n_u, n_p), adv, Fu)
            if self._load is not None:                                         # body force: F_u -= (f, v)
                self.ctx.axpy(Fu, self._dload, -1.0, n=n_u)
            fin.zero_bc(Fu)                                                    # bc.zero(F), solver.py:282-286
            self._dB.mult(st, hip.view(self._dF, n_u, n_p))                   # F_p = B u

    def _set_parameters(self):
        with self._on_stream():
            for T, dt in self._device_transfers:                            # AutoSchoeberlTransfer.rebuild, transfer.py:173-184
                if T.nu != self.nu:
                    T.nu = self.nu
                    dt.update(self.nu, self.gamma)
        self.saddle.update(self.nu, self.gamma)

    def _device_winds(self):
        """GLS's wind on every level: the resident finest velocity copied, the coarser ones injected as the state is."""
        self.ctx.copy(self._dwind[-1], self._dstate[-1], n=self.n_u)
        for l in range(len(self.levels) - 1, 0, -1):
            self.hmg.mg.transfers[l - 1].inject(self._dwind[l], self._dwind[l - 1])

    # -- the device-resident state: (u | p) on one GPU, (owned u | owned p) per rank on partitions -----------------------------
    # (``_own_dofs`` / ``_own_cells`` index the rank's entries of a global velocity / pressure vector, ``_n_own`` / ``_np_own``
    # count them, ``_ksp`` is the library's outer solver: set by ``_create_device``)
    def _push_state(self):
        u, p = self._host_u[self._own_dofs], self._host_p[self._own_cells]
        with self._on_stream():
            self._dz.set(np.concatenate([u, p, np.zeros(self._dz.n - u.size - p.size)]))

    def _push_load(self):
        if getattr(self, "_dload", None) is None:
            self._dload = self.ctx.vec(max(self._n_own, 1))
        with self._on_stream():
            self._dload.set(np.ascontiguousarray(self._load[self._own_dofs]) if self._n_own else np.zeros(1))

    def _zdot(self, x, y):
        with self._on_stream():
            return self._ksp.dot(x, y)

    def _zsolve(self, b, x):
        with self._on_stream():
            return self._ksp.solve(b, x, self.rtol, self.atol, self.params["ksp_max_it"], 30)

    def _zaxpy(self, y, x, a):
        with self._on_stream():
            self.ctx.axpy(y, x, a, n=self._n_own + self._np_own)

    def _shift_pressure(self):
        """p -= (int p) / |domain| on the device."""
        n_u, n_p = self._n_own, self._np_own
        if getattr(self, "_dvolz", None) is None:
            with self._on_stream():
                self._dvolz = self.ctx.vec(np.concatenate([np.zeros(n_u), self.vol[self._own_cells],
                                                           np.zeros(self._dz.n - n_u - n_p)]))
                self._dones = self.ctx.vec(np.ones(max(n_p, 1)))
        c = self._zdot(self._dvolz, self._dz) / self.area
        with self._on_stream():
            self.ctx.axpy(self._dz, self._dones, -c, n=n_p, y_off=n_u)

    def _device_state_resident(self):
        """Whether the Newton loop runs with the state on the device (the operators are refreshed there anyway)."""
        return self.device_assembly

    def _linear_solve(self, rhs):
        """J d = rhs for the current operators: (d, Krylov iterations, true residual norm)."""
        db, dx = self.ctx.vec(rhs), self.ctx.vec(self.n_u + self.n_p)
        its, rn = self.saddle.solve(db, dx, self.rtol, self.atol, self.params["ksp_max_it"], 30)
        return dx.get(), its, rn

    def close(self):
        if getattr(self, "_asm_ready", False):
            self._dB.close()
            self._dBT.close()
        self.saddle.close()
        self.hmg.mg.close()

    # -- host side: state on all levels, operators, residual -------------------------------------------------------------
    def _winds(self, u):
        """Current velocity as nodal field on every level (finest given, coarser by inject, solver.py:595)."""
        d = self.problem.dim
        w = [None] * len(self.levels)
        w[-1] = u.reshape(-1, d)
        for l in range(len(self.levels) - 1, 0, -1):
            T = self.transfers[l - 1]
            # nested uniform hierarchy: every coarse node is a fine node; bary hierarchy: point evaluation (sv.bary_injection)
            w[l - 1] = w[l][T.inject_map] if T.inject_map is not None else T.inject_matrix @ w[l]
        return w

    def level_values(self, L, state, adv, with_bc):
        """BSR values of the linearised momentum block of level L about ``state`` (num_nodes, dim): viscous + grad-div +
        Newton-linearised advection (+ the linearised SUPG term, ``advect * stabilisation_form``, solver.py:233-234)."""
        state = np.ascontiguousarray(state)
        A = _assemble(L, self.nu, self.gamma, adv, state, False, self.sv)
        fq = self._fq[L.level] if self._fq is not None else None
        if adv and self.supg:
            _hostlib.supg(L.V, state, self.nu, self.supg_weight, self.supg_magic, L.A.rowptr, L.A.colidx, A, fq=fq)
        if adv and self.gls:          # the wind of this solve (the state itself before any solve)
            wind = self._host_winds[L.level] if self._host_winds is not None else state
            _hostlib.gls(L.V, state, wind, self.nu, self.supg_weight, self.supg_magic, L.A.rowptr, L.A.colidx, A, fq=fq)
        L.facet_beta = None
        if adv and self.burman:
            beta = np.empty(L.facets.nf)
            self._host_burman(L)(state, adv * self.burman_weight, vals=A, beta=beta)
            L.facet_beta = (beta, adv * self.burman_weight)      # for PCPATCH's facet rule in the patch factorisation
        if with_bc:
            _hostlib.apply_bc_bsr(L.V.num_nodes, L.V.dim, L.A.rowptr, L.A.colidx, A, np.repeat(L.V.bc_node_mask, L.V.dim))
        return A

    def _host_burman(self, L):
        """The host pass of the Burman term on level L (its contributor lists built once)."""
        cache = self.__dict__.setdefault("_host_burman_cache", {})
        if L.level not in cache:
            from .burman import HostBurman
            cache[L.level] = HostBurman(L)
        return cache[L.level]

    def _rediscretise(self, u, adv):
        if self.device_assembly:
            return self._rediscretise_device(u, adv)
        winds = self._winds(u)
        for L, w in zip(self.levels, winds):
            if self.allu and L is not self.levels[-1]:      # allu solves with the finest operator alone
                continue
            L.A = BSR(L.A.nbrows, L.A.nbcols, L.bs, L.A.rowptr, L.A.colidx, self.level_values(L, w, adv, True))
            L.nu = self.nu
        self._push_operators()

    def residual(self, u, p, adv):
        """F(u, p) of solver.py:565-568 (rhs = 0), Dirichlet rows zeroed (``bc.zero(F)``, solver.py:282-286)."""
        if self.device_assembly:
            return self._residual_device(u, p, adv)
        L = self.levels[-1]
        d = self.problem.dim
        wind = np.ascontiguousarray(u.reshape(-1, d))
        A0 = BSR(L.A.nbrows, L.A.nbcols, L.bs, L.A.rowptr, L.A.colidx,
                 _assemble(L, self.nu, self.gamma, 0.0, None, False, self.sv)).to_scipy()
        Fu = A0 @ u
        if adv:
            J = BSR(L.A.nbrows, L.A.nbcols, L.bs, L.A.rowptr, L.A.colidx,
                    _assemble(L, self.nu, self.gamma, 1.0, wind, False, self.sv)).to_scipy()
            Fu = 0.5 * (Fu + J @ u)                  # A0 u + 1/2 N(u) u with N = J - A0
            fq = self._fq[L.level] if self._fq is not None else None
            if self.supg:
                Fs = np.zeros_like(Fu)
                _hostlib.supg(L.V, wind, self.nu, self.supg_weight, self.supg_magic, F=Fs, fq=fq)
                Fu = Fu + Fs
            if self.gls:
                Fs = np.zeros_like(Fu)
                W = self._host_winds[-1] if self._host_winds is not None else wind
                _hostlib.gls(L.V, wind, W, self.nu, self.supg_weight, self.supg_magic, F=Fs, fq=fq)
                Fu = Fu + Fs
            if self.burman:
                Fb = np.zeros_like(Fu)
                self._host_burman(L)(wind, adv * self.burman_weight, F=Fb)
                Fu = Fu + Fb
        Fu = Fu + self.B_raw.T @ p
        if self._load is not None:                   # body force (manufactured solutions, examples/mms.py): F_u -= (f, v)
            Fu = Fu - self._load
        Fu[L.bc_dofs] = 0.0
        Fp = self.B_raw @ u
        return Fu, Fp

    def _stabilisation_load(self, f):
        """The body force at the SUPG / GLS points of every level (it depends on Re: once per solve), to the device levels when
        they refresh their operators."""
        if self._partitioned:
            raise NotImplementedError("a body force with SUPG on partitioned levels: the rank-local load tables are not built")
        self._fq = [hip.supg_load(L.V, f) for L in self.levels]
        if self.device_assembly:
            for fq, dl in zip(self._fq, self.hmg.mg.levels):
                dl.set_supg_load(fq)

    # -- adjoint (alfi/solver.py:520-535; alfi_amd.adjoint) -----------------------------------------------------------------
    def setup_adjoint(self, J):
        """Keep the functional J (``value(solver, u, p)``, ``gradient(solver, u, p) -> (g_u, g_p or None)``) and create
        ``self.solver_adjoint``, whose ``solve(rtol=None, atol=None)`` writes ``self.z_adj = (lam_u, lam_p)`` for the state of
        the last ``solve(re)``: J_F(z)^T z_adj = -dJ/dz with homogeneous Dirichlet conditions."""
        from .adjoint import setup_adjoint
        return setup_adjoint(self, J)

    def solve_adjoint(self, J, rtol=None, atol=None):
        """``setup_adjoint(J)`` and one adjoint solve: returns (z_adj, info).  J a list or tuple of functionals: ONE refresh,
        transpose and factorisation and one block solve; z_adj is then a list of (lam_u, lam_p), and ``linear_iter``,
        ``residual_norm``, ``rhs_norm`` and ``converged`` of info are lists."""
        info = self.setup_adjoint(J).solve(rtol=rtol, atol=atol)
        return self.z_adj, info

    # -- the solve loop ---------------------------------------------------------------------------------------------------
    def solve(self, re):
        t0 = time.time()
        if re == 0:
            adv, self.nu = 0.0, self.char_L * self.char_U                   # Stokes, solver.py:261-264
        else:
            adv, self.nu = 1.0, self.char_L * self.char_U / re
        self._last_solve = (re, adv)
        self._set_parameters()
        self._load = None
        self._fq = None
        if hasattr(self.problem, "rhs"):             # NavierStokesProblem.rhs (problem.py:46-47 of the reference): default none
            from .mms import load_vector
            f = lambda x: self.problem.rhs(x, re)
            self._load = load_vector(self.levels[-1].V, f)
            if self.supg or self.gls:     # the strong residual carries the force too (solver.py:216-217): per level, per solve
                self._stabilisation_load(f)
        resident = self._device_state_resident()
        if resident:
            if not (self._device_newer or self._device_current):
                self._push_state()
                self._device_current = True
            if self._load is not None:
                self._push_load()
            if self.gls:              # the wind: z_last, the state at the start of this solve (solver.py:199, 205, 215)
                self._device_winds()
        elif self.gls:                # ... on every level, on the host
            self._host_winds = [np.ascontiguousarray(w) for w in self._winds(self.u.copy())]
        return self._newton((_DeviceState if resident else _HostState)(self, adv), re, t0)

    def _newton(self, state, re, t0):
        """``snes_type newtonls`` with the basic line search around a state (``_HostState`` / ``_DeviceState``):
        ``residual()`` evaluates F at the iterate and returns |F|, ``step()`` takes one Newton step and returns (Krylov
        iterations, linear residual norm, |step|, |iterate|), ``finish()`` publishes the iterate and returns what ``solve``
        returns as z."""
        lin_its, newton_its, small_step = 0, 0, False
        with self._timed("residual_s"):
            f0 = fnorm = state.residual()
        tol = max(self.snes_rtol * f0, self.snes_atol)
        hist = [fnorm]
        while fnorm > tol and newton_its < self.snes_max_it and not small_step:
            its, rn, snorm, znorm = state.step()
            lin_its += its
            newton_its += 1
            self.timings["newton_steps"] += 1
            with self._timed("residual_s"):
                fnorm = state.residual()
            hist.append(fnorm)
            # SNESConvergedDefault [3P] with snes_stol (solver.py:490, 498): the step is small relative to the iterate
            small_step = snorm < self.snes_stol * znorm
            if self.verbose:
                print("[alfi_amd] Re %g  Newton %d  |F| %.3e  (%d Krylov its, linear residual %.2e)"
                      % (re, newton_its, fnorm, its, rn), flush=True)
        z = state.finish()
        info = {"Re": re, "nu": self.nu, "linear_iter": lin_its, "nonlinear_iter": newton_its,
                "time": (time.time() - t0) / 60.0, "residual_history": hist, "converged": small_step or fnorm <= tol,
                "converged_reason": "SNORM_RELATIVE" if small_step else "FNORM"}
        return z, info


class _HostState(object):
    """The Newton iterate as host arrays (``device_assembly=False``): J d = -F, z += d."""

    def __init__(self, solver, adv):
        self.s, self.adv = solver, adv
        self.u, self.p = solver.u.copy(), solver.p.copy()

    def residual(self):
        self.Fu, self.Fp = self.s.residual(self.u, self.p, self.adv)
        return float(np.sqrt(self.Fu @ self.Fu + self.Fp @ self.Fp))

    def step(self):
        s, u, p = self.s, self.u, self.p
        s._rediscretise(u, self.adv)
        rhs = -np.concatenate([self.Fu, self.Fp])
        with s._timed("solve_s"):
            delta, its, rn = s._linear_solve(rhs)
        u += delta[:s.n_u]
        p += delta[s.n_u:]
        return its, rn, np.linalg.norm(delta), float(np.sqrt(u @ u + p @ p))

    def finish(self):
        s = self.s
        if s.nullspace:
            self.p -= (s.vol @ self.p) / s.area                              # zero pressure integral, solver.py:273-277
        s.u, s.p = self.u, self.p
        return self.u, self.p


class _DeviceState(object):
    """The Newton iterate, the residual and the update resident in HBM (``_dz``, ``_dF``, ``_dd``): per step the operators are
    refreshed from the state in place, J e = F is solved on the device (e = - update; the Krylov iterates of b and - b mirror
    each other), z -= e, and only scalars -- norms, iteration counts -- reach the host."""

    def __init__(self, solver, adv):
        self.s, self.adv = solver, adv

    def _norm(self, v):
        return float(np.sqrt(self.s._zdot(v, v)))

    def residual(self):
        self.s._residual_on_device(self.adv)
        return self._norm(self.s._dF)

    def step(self):
        s = self.s
        s._rediscretise_device(None, self.adv)
        with s._timed("solve_s"):
            its, rn = s._zsolve(s._dF, s._dd)
            s._zaxpy(s._dz, s._dd, -1.0)
            s._device_newer, s._device_current = True, False
        return its, rn, self._norm(s._dd), self._norm(s._dz)

    def finish(self):
        s = self.s
        if s.nullspace:                                                      # zero pressure integral, solver.py:273-277
            s._shift_pressure()
            s._device_newer, s._device_current = True, False
        return _StateHandle(s)


class _StateHandle(object):
    """What ``solve`` returns for the state while it lives on the device (the reference returns the Function z, a handle as
    well): unpacking it -- ``u, p = z`` -- fetches the arrays."""

    def __init__(self, solver):
        self._s = solver

    def __iter__(self):
        return iter((self._s.u, self._s.p))


def run_solver(solver, res):
    """alfi.driver.run_solver (driver.py:95-128) without checkpoints / ParaView output: continuation in Re."""
    results = {}
    for re in res:
        _, results[re] = solver.solve(re)
    return results


# PETSc event names the reference's report prints (driver.py:80) -> the library's profiling classes
from ._lib import PETSC_EVENT_NAMES as _PETSC
_EVENT_NAMES = [(_PETSC[k], k) for k in ("PATCH_APPLY", "PATCH_SCATTER", "PATCH_FACTOR", "MATMULT", "BLAS1", "PROLONG", "RESTRICT",
                                         "COARSE")]


def performance_info(solver, out=print):
    """alfi.driver.performance_info (driver.py:77-92): device time per event class since profiling was switched on
    (``solver.ctx.prof_enable(True)`` before the solves), sorted, with time per 1k dofs."""
    prof = solver.ctx.prof_get()
    ndofs = solver.n_u + solver.n_p
    rows = sorted(((name, prof[key][0] * 1e-3, prof[key][1]) for name, key in _EVENT_NAMES), key=lambda r: -r[1])
    out("Some performance info:")
    for name, t, cnt in rows:
        out(("%s:" % name).ljust(30) + "Time = % 6.2fs, Time/1kdofs = %.2fs  (%d launches)" % (t, 1000 * t / ndofs, cnt))
    return rows
