"""The Newton / Reynolds-continuation loop of alfi_amd.nssolver with the device side on partitioned levels (one process per
GPU): ``DistNavierStokesSolver`` puts ``HipNavierStokesSolver`` on ``DistMultigrid`` + ``DistSaddle`` (alfi_amd.dist), and
``StateExchange`` feeds the refresh of every rank's level operators from the Newton state distributed over the devices.

A module of its own because it needs the single-GPU solver, the library wrappers and torch, which the partitioning of
alfi_amd.dist alone does not; ``alfi_amd.dist.DistNavierStokesSolver`` / ``alfi_amd.dist.StateExchange`` import it on first
use."""

import numpy as np
import torch

from . import _hostlib, env, hip
from .dist import DistMultigrid, DistSaddle, FacetPart, HaloBuffers, assembly_cells, local_host_operator, localize_pressure
from .lazy import LazyOperator, _row_map, _take_rows
from .nssolver import HipNavierStokesSolver
from .problem import BSR


class _StatePart(object):
    """What HaloBuffers reads of a LevelPart."""

    def __init__(self, bs, send_counts, recv_counts):
        self.bs, self.send_counts, self.recv_counts = bs, send_counts, recv_counts


def composed_injection(transfers, nlev, level, rows, n_fine=None):
    """Rows ``rows`` of I_level . I_level+1 ... I_nlev-2 (scipy CSR, len(rows) x finest nodes): the nodal values of ``level`` as a
    linear map of the finest field, the composition of the ``inject`` maps (alfi/solver.py:595).  I_l is ``inject_matrix`` of
    transfers[l] -- the point evaluation of the barycentric hierarchy, sv.bary_injection -- or, where ``inject_map`` is set
    (nested hierarchies: a coarse node IS a fine node), the 0/1 matrix of that map.  Formed from the top down through the rows
    actually needed, C_l[rows] = I_l[rows] . C_l+1[columns of I_l[rows]]: no global product, the cost follows len(rows).  The
    finest level gives identity rows.  Column indices sorted, duplicates summed, nothing eliminated afterwards (the sparse
    product itself leaves out a sum that cancels to exactly 0.0).  Device-free.
    n_fine: the finest level's node count; read off the last transfer when not given (a single level has none: give it)."""
    import scipy.sparse as sp
    rows = np.asarray(rows, dtype=np.int64)
    if level == nlev - 1:
        if n_fine is None:
            T = transfers[nlev - 2]           # its fine space, or the block rows of its prolongation: the finest nodes
            n_fine = T.Vf.num_nodes if hasattr(T, "Vf") else T.P.nbrows
        return sp.csr_matrix((np.ones(rows.size), rows, np.arange(rows.size + 1)), shape=(rows.size, n_fine))
    T = transfers[level]
    imap = getattr(T, "inject_map", None)
    if imap is not None:              # rows of a 0/1 matrix select rows of the next composition
        return composed_injection(transfers, nlev, level + 1, np.asarray(imap, dtype=np.int64)[rows], n_fine)
    I = sp.csr_matrix(T.inject_matrix)[rows]
    cols = np.unique(I.indices)
    C = composed_injection(transfers, nlev, level + 1, cols, n_fine)
    I = sp.csr_matrix((I.data, np.searchsorted(cols, I.indices), I.indptr), shape=(rows.size, cols.size))
    out = (I @ C).tocsr()
    out.sum_duplicates()
    out.sort_indices()
    return out


def _is_index_map(C):
    """A composed injection whose rows all have one entry of weight exactly 1.0: an index gather."""
    return C.nnz == C.shape[0] and np.array_equal(C.indptr, np.arange(C.shape[0] + 1)) and bool((C.data == 1.0).all())


class StateExchange(object):
    """The distributed Newton state as input of the rank's operator refresh: every level's state vector (the level's local
    nodes and the ring of nodes of the cells around them, alfi_level_set_assembly; with Burman terms also the nodes of the
    facets' off-rank cells) filled ON THE DEVICE from the velocity the ranks own on the finest level -- one halo exchange per
    refresh, then one gather per level.  A level's state is the composition of the ``inject`` maps (alfi/solver.py:595) applied
    to the finest velocity, ``composed_injection`` over the level's state nodes: on the nested hierarchies a node of level l IS a
    node of the finest level and the gather is an index gather (alfi_vec_gather); on the barycentric hierarchy of the
    Scott-Vogelius pair a node of level l is a point evaluation of the finest field, a few weights per row, and the gather is
    the weighted one (alfi_vec_gather_csr).  Levels whose composed map is an index map -- the finest always -- take the index
    gather on either hierarchy.
    The exchange runs through a level that exists only for its halo plan (identity operator): owned block = the rank's owned
    finest nodes in the finest level's local order, ghosts = every other finest node some level's refresh reads here; it
    therefore takes whichever transport the multigrid levels take (the library's RCCL communicator, or the callback)."""

    def __init__(self, dmg, levels, transfers, asm_nodes, device):
        """asm_nodes[i]: global node ids (numbering of level dmg.lmin + i) of the state entries of local level i, or None."""
        p = dmg.fine.part
        bs, rank, world = p.bs, dmg.comm.rank, dmg.comm.world
        nlev = len(levels)
        n_fine = levels[-1].A.nbrows
        # need[i]: local level i's state as rows over the finest nodes (rank-local: the rows this rank reads, nothing global)
        need = [None if a is None else composed_injection(transfers, nlev, dmg.lmin + i, a, n_fine)
                for i, a in enumerate(asm_nodes)]
        allneed = np.unique(np.concatenate([C.indices for C in need if C is not None] + [np.zeros(0, dtype=np.int64)]))
        allneed = allneed.astype(np.int64)
        ghosts = allneed[(allneed < p.lo) | (allneed >= p.hi)]               # ascending => grouped by owner
        owner = np.searchsorted(p.splits, ghosts, side="right") - 1
        recv_counts = np.bincount(owner, minlength=world).astype(np.int64)
        off = np.concatenate([[0], np.cumsum(recv_counts)])
        wanted = dmg.comm.all_gather_object([ghosts[off[q]:off[q + 1]] for q in range(world)])
        send_lists = [p.own_perm[np.asarray(wanted[q][rank], dtype=np.int64) - p.lo] for q in range(world)]
        send_counts = np.array([len(x) for x in send_lists], dtype=np.int64)
        send_nodes = np.concatenate(send_lists).astype(np.int32) if send_counts.sum() else np.zeros(0, dtype=np.int32)
        nb = p.nb_own + len(ghosts)
        ctx = dmg.ctx
        A = BSR(nb, nb, bs, np.arange(nb + 1, dtype=np.int32), np.arange(nb, dtype=np.int32), np.tile(np.eye(bs), (nb, 1, 1)))
        self.level = hip.Level(ctx, A, np.zeros(0, dtype=np.int32))
        if dmg.transport == "rccl":
            self.level.set_partition(p.nb_own, True, send_nodes, None, None, len(ghosts))
            nbr = np.flatnonzero((send_counts > 0) | (recv_counts > 0))
            self.level.set_neighbours(nbr, send_counts[nbr], recv_counts[nbr])
        else:
            hb = HaloBuffers(_StatePart(bs, send_counts, recv_counts), device)
            self.level.set_partition(p.nb_own, True, send_nodes, hb.sendbuf.data_ptr(), hb.recvbuf.data_ptr(), len(ghosts))
            dmg.halos[self.level.id] = hb
        self.ctx, self.bs, self.n_own = ctx, bs, p.nb_own * bs
        self.vec = ctx.vec(max(nb * bs, 1))
        # position of a finest node in that vector: owned -> its local index, ghost -> behind the owned block
        def pos(g):
            g = np.asarray(g, dtype=np.int64)
            own = (g >= p.lo) & (g < p.hi)
            out = np.empty(g.shape[0], dtype=np.int64)
            out[own] = p.own_perm[g[own] - p.lo]
            out[~own] = p.nb_own + np.searchsorted(ghosts, g[~own])
            return out
        # per level: an index list (alfi_vec_gather), or (rowptr, colidx, weights) in CSR order (alfi_vec_gather_csr)
        self.idx, self.csr = [], []
        for C in need:
            index = C is not None and _is_index_map(C)
            self.idx.append(ctx.ivec(pos(C.indices)) if index else None)
            self.csr.append(None if C is None or index else
                            (ctx.ivec(C.indptr), ctx.ivec(pos(C.indices)), ctx.vec(C.data if C.nnz else np.zeros(1))))
        self.bytes_received = int(len(ghosts)) * bs * 8

    def refresh(self, du_owned, states):
        """du_owned: device vector that starts with the rank's owned finest velocity; states[i]: device state of local level i."""
        self.ctx.copy(self.vec, du_owned, n=self.n_own)
        self.level.halo_forward(self.vec)
        for ix, csr, st in zip(self.idx, self.csr, states):
            if ix is not None:
                self.ctx.gather(st, self.vec, ix, self.bs)
            elif csr is not None:
                self.ctx.gather_csr(st, self.vec, csr[0], csr[1], csr[2], self.bs)

    def close(self):
        self.level.close()


class DistNavierStokesSolver(HipNavierStokesSolver):
    """HipNavierStokesSolver with the device side on partitioned levels (one process per GPU): DistMultigrid + DistSaddle.
    Every rank rediscretises ITS OWN rows of the level operators -- on its device from the cells that touch its nodes
    (``_rediscretise_device``; on its host cores only with ALFI_DEVICE_ASSEMBLY=0).  The Newton state is DISTRIBUTED on the
    devices for every discretisation, every rank its owned velocity and pressure dofs (``StateExchange`` feeds the levels'
    refresh states from it -- index gathers on the nested hierarchies, weighted gathers of the composed point evaluations on the
    barycentric hierarchy of the Scott-Vogelius pair; ``u`` / ``p`` gather it, collectively, when somebody asks); the
    host-assembly path and ``device_state=False`` keep a replicated host state.  The Burman terms of the Scott-Vogelius pair are formed by every rank
    over the facets of its cells (``FacetPart``), on the device or, with ALFI_DEVICE_ASSEMBLY=0, by the host pass."""

    _partitioned = True

    def __init__(self, *args, min_dofs=400000, group=None, device_state=True, condense_min_bytes=None, **kwargs):
        """device_state False: the Newton state replicated on the hosts, every level's state formed there (``_winds``) and
        uploaded, residual and update gathered after every step (the loop of round 4; kept for comparisons).
        condense_min_bytes: DistMultigrid's (None: the library's default threshold for condensing vertex-star factors)."""
        self._min_dofs, self._group, self._want_device_state = min_dofs, group, bool(device_state)
        self._condense_min_bytes = condense_min_bytes
        super().__init__(*args, **kwargs)

    def _device_state_resident(self):
        # the state lives distributed on the devices -- every rank its owned velocity and pressure dofs (P0: its cells', the
        # Scott-Vogelius pair: the P_{k-1}^dg rows of its cells) -- whenever the operators are refreshed there
        return self.device_assembly and getattr(self, "_exch", None) is not None

    def _any_rank(self, flag):
        return any(self.dmg.comm.all_gather_object(bool(flag)))

    def _on_stream(self):
        return torch.cuda.stream(self.dmg.stream)

    def _lazy_generation(self):
        # rank-local generation: every rank assembles the operator / transfer rows of its partition only (config 4 on 8
        # ranks: 4.5 GB of host memory per rank instead of 25).  The HOST refresh of SUPG terms works on global values: with
        # SUPG the generation is rank-local only while the operators are refreshed on the device (the default).
        return (not self.supg or self.device_assembly) and not env.dist_global_generation()

    def _create_device(self, restriction):
        self.dmg = DistMultigrid(self.levels, self.transfers, self.params["fieldsplit_0"]["mg_levels"]["ksp_max_it"],
                                 robust_restriction=restriction, group=self._group, min_dofs=self._min_dofs,
                                 full_cycle=self.params["fieldsplit_0"].get("pc_mg_type") == "full",
                                 condense_min_bytes=self._condense_min_bytes, patch_factor_dtype=self._patch_factor_dtype,
                                 macro_factor_dtype=self._macro_factor_dtype)
        self.ctx = self.dmg.ctx
        L = self.levels[-1]
        self.saddle = sad = DistSaddle(self.dmg, self.B, self.vol, L.V.cell_nodes, self.nu, self.gamma,
                                       remove_constant_nullspace=self.nullspace, mass_inv=self.Minv if self.sv else None)
        # transfers present on this rank link local levels lmin.. ; their (nu, gamma) follow the solver's
        self._ksp, self._device_transfers = sad.sad, list(zip(self.dmg.local_transfers, self.dmg.mg.transfers))
        self._own_dofs, self._own_cells = self.dmg.fine.part.own_dofs(), sad.cells
        self._n_own, self._np_own = sad.n_own, sad.np_own
        self._facet_parts = {}
        if self.burman:
            # every level with owned rows: the rank's facets; levels with owned patches: PCPATCH's facet rule for them
            # (the patches were factored from the Stokes operators, which hold no Burman part: the rule applies from the
            # first refresh with adv > 0 on)
            with self._on_stream():
                for dl, LL in zip(self.dmg.levels, self.dmg.local_levels):
                    if LL.part.nb_own == 0:
                        continue
                    Lg = self.levels[LL.level]
                    fp = self._facet_parts[LL.level] = FacetPart(Lg.V, Lg.facets, LL.part)
                    if LL.level > 0:
                        dl.set_patch_facet_correction(fp.table.nf, *fp.patch_facet_corrections(Lg.V, Lg.facets, LL))

    def _push_operators(self):
        self.dmg.update(self.levels)

    def setup_adjoint(self, J):
        """``solver_adjoint`` on partitioned levels: with the operators refreshed on the device every rank forms its own rows
        of J^T (the transposed refresh, alfi_amd.adjoint).  Host assembly (ALFI_DEVICE_ASSEMBLY=0, a fallback to it, a solver
        never set up) stays refused: there J^T needs the mirror block of every ghost column, and those belong to other
        ranks.  The check comes before any collective and every rank reaches the same verdict."""
        if not (getattr(self, "_asm_ready", False) and getattr(self, "device_assembly", False)):
            raise NotImplementedError("adjoint solves on partitioned levels need the device-side operator refresh: with host "
                                      "assembly J^T needs the mirror block of every ghost column, and those belong to other "
                                      "ranks")
        from .adjoint import setup_adjoint
        return setup_adjoint(self, J)

    def _supg_host_needs_global_values(self):
        if isinstance(self.levels[-1].A, LazyOperator):
            raise RuntimeError("SUPG on partitioned levels without the device-side operator refresh needs the global "
                               "operator values: start with ALFI_DIST_GLOBAL_GENERATION=1 (the hierarchy was generated "
                               "rank-locally because the device refresh was expected to be available)")

    # -- operator refresh on the device, every rank its own rows (alfi/solver.py:320, 325 under solver.py:604-605) --------------
    def _setup_device_assembly(self):
        """Once per solver, RANK-LOCAL (no collective: ``_start_device_assembly`` agrees on the outcome afterwards): every local
        level with owned rows gets the cells that touch its local nodes and the contributor lists of its local sparsity
        (alfi_level_set_assembly on a partitioned level: every term of the operator is formed on the device, cell by cell);
        the state of a Newton step then reaches every level's state vector -- local nodes and the ring of nodes around them, a
        few megabytes -- through ``StateExchange`` (``device_state=False``: uploaded from the replicated host state) and the
        operators are rebuilt from it on the device.  Every discretisation the single-GPU solver refreshes on the device: the
        P0-pressure pairs, the Scott-Vogelius pair with or without Burman terms and the SUPG terms (element matrices of the rank's
        cells -- all cells that touch a local node -- gathered into the rank's rows).
        Ranks that hold only ghost copies of a level (the coarse side of the first distributed transfer) skip it: no patch
        and no product reads those rows."""
        dmg = self.dmg
        self._asm = []
        with self._on_stream():
            for dl, LL in zip(dmg.levels, dmg.local_levels):
                p = LL.part
                if p.nb_own == 0:
                    self._asm.append(None)
                    continue
                L = self.levels[LL.level]
                V = L.V
                fp = self._facet_parts.get(LL.level)
                if fp is not None:               # the facet-coupled sparsity has blocks no cell contributes to
                    dl.set_facet_blocks(True)
                    cells, cn, nodes = fp.cells, fp.cell_nodes, fp.state_nodes
                else:
                    cells, cn, nodes = assembly_cells(V, p)
                dl.set_assembly(V, LL.A.rowptr, LL.A.colidx, full_div=self.sv, cells=cells, cell_nodes=cn)
                bcn = np.flatnonzero(V.bc_node_mask[p.nodes])              # Dirichlet nodes among ALL local nodes
                dl.set_assembly_bc((bcn[:, None] * L.bs + np.arange(L.bs)).ravel())
                if self.supg:
                    dl.set_supg(V, cells=cells)
                if fp is not None:               # the rank's facets; the state grows by their off-rank cells' nodes
                    dl.set_burman(fp.table, LL.A.rowptr, LL.A.colidx, lists=fp.lists(LL.A))
                assert dl.assembly_state_size() == nodes.size * L.bs
                self._asm.append((nodes, self.ctx.vec(dl.assembly_state_size())))
            L = self.levels[-1]
            self._dres = self.ctx.vec(dmg.n_loc)
            # the residual's divergence products with ALL columns of B (the Jacobian's B, Dirichlet columns zeroed, lives
            # in the saddle solver): the rank's cells over its local velocity dofs
            rows, Bloc, _, _ = localize_pressure(self.B_raw, None, L.V.cell_nodes, dmg.fine.part, L.bs)
            self._res_rows = rows
            self._dB = hip.Csr(self.ctx, Bloc)
            self._dBT = hip.Csr(self.ctx, Bloc.T.tocsr())
            self._dp, self._dFp = self.ctx.vec(max(len(rows), 1)), self.ctx.vec(max(len(rows), 1))
            self._dwc = self.ctx.vec(dmg.n_loc)
            self._exch = None
            # the residual's pressure rows are the outer solve's (P0: the rank's cells; Scott-Vogelius: npc rows per cell)
            assert np.array_equal(self._res_rows, self.saddle.cells)
            if self._want_device_state:
                # the distributed device-resident state: (owned velocity | owned pressure) per rank
                n = self.saddle.n
                self._dz, self._dF, self._dd = self.ctx.vec(n + 1), self.ctx.vec(n + 1), self.ctx.vec(n + 1)
        self._asm_ready = True

    def _setup_state_exchange(self):
        """COLLECTIVE, and so a phase of its own, entered only once every rank has the rank-local part: the exchange that
        feeds every level's refresh from the distributed state (its gather of the ghost lists comes before any device call of
        its own)."""
        if self._want_device_state:
            with self._on_stream():
                self._exch = StateExchange(self.dmg, self.levels, self.transfers,
                                           [None if a is None else a[0] for a in self._asm], self.dmg.device)

    def _device_levels(self):
        # (levels without owned rows are skipped)
        return [(dl, asm[1], None) for asm, dl in zip(self._asm, self.dmg.levels) if asm is not None]

    def _refresh_states(self):
        self._exch.refresh(self._dz, [None if a is None else a[1] for a in self._asm])

    def _upload_states(self, u):
        for asm, w in zip(self._asm, self._winds(u)[self.dmg.lmin:]):
            if asm is not None:
                asm[1].set(np.ascontiguousarray(w[asm[0]]).ravel())

    def _device_states(self, u):
        if u is None:                 # the state lives on the devices: one exchange feeds every level's refresh
            self._refresh_states()
        else:
            self._upload_states(u)

    def _factor_levels(self):
        for L in self.levels:
            L.nu = self.nu
        self.dmg.refactor(self.levels)
        self.ctx.sync()

    # -- the distributed device-resident state ------------------------------------------------------------------------------
    def _fetch_state(self):
        """COLLECTIVE: every rank contributes its owned entries (``u`` / ``p`` after a solve must be read on all ranks)."""
        if self._device_newer:
            sad = self.saddle
            with self._on_stream():
                z = self._dz.get()
            u, p = np.zeros(self.n_u), np.zeros(self.n_p)
            for dofs, cells, zu, zp in self.dmg.comm.all_gather_object((self._own_dofs, sad.cells, z[:sad.n_own],
                                                                        z[sad.n_own:sad.n])):
                u[dofs] = zu
                p[np.asarray(cells)] = zp
            self._host_u, self._host_p = u, p
            self._device_newer, self._device_current = False, True

    def _owners_BTp(self, fin, dp):
        """``_dwc`` = B^T p on the owners: the rank's cells' share, the ghost rows' part reverse-added over the halo."""
        self._dBT.mult(dp, self._dwc)
        fin.halo_reverse_add(self._dwc)

    def _momentum_residual(self, fin, st, wind, dp, adv, Fu):
        self._velocity_residual(fin, st, wind, adv, self._dres)
        self._owners_BTp(fin, dp)
        self.ctx.copy(Fu, self._dres, n=self._n_own)
        self.ctx.axpy(Fu, self._dwc, 1.0, n=self._n_own)

    def _residual_on_device(self, adv):
        """The rank's rows of F(z) for the distributed state: the state of the finest level's refresh comes through the
        exchange, the matrix-free product and the divergence products run over the rank's cells."""
        with self._on_stream():
            self._refresh_states()
        super()._residual_on_device(adv)

    def _residual_device(self, u, p, adv):
        """The rank's rows of F_u = (nu K + gamma D + 1/2 N(u)) u + B^T p on the device -- one matrix-free product over the
        rank's cells (alfi_level_assemble_mult: the state carries the ring of nodes around the local ones, no exchange),
        the rank's cells' share of B^T p reverse-added onto the owners -- and its rows of F_p = B u; the pieces are then
        gathered (the Newton state is replicated)."""
        L = self.levels[-1]
        dmg, fin = self.dmg, self.dmg.levels[-1]
        nodes, st = self._asm[-1]
        n_own = dmg.n_own
        with self._on_stream():
            st.set(np.ascontiguousarray(u.reshape(-1, L.bs)[nodes]).ravel())
            self._velocity_residual(fin, st, None, adv, self._dres)
            self._dp.set(np.ascontiguousarray(p[self._res_rows]) if len(self._res_rows) else np.zeros(1))
            self._owners_BTp(fin, self._dp)
            self._dB.mult(st, self._dFp)
            f_own = self._dres.get()[:n_own] + self._dwc.get()[:n_own]
            fp_own = self._dFp.get()[:len(self._res_rows)]
        Fu, Fp = np.zeros(self.n_u), np.zeros(self.n_p)
        for dofs, f, rows, fp in dmg.comm.all_gather_object((self._own_dofs, f_own, self._res_rows, fp_own)):
            Fu[dofs] = f
            Fp[rows] = fp
        if self._load is not None:
            Fu -= self._load
        Fu[L.bc_dofs] = 0.0
        return Fu, Fp

    # -- host assembly (ALFI_DEVICE_ASSEMBLY=0), every rank its own rows ------------------------------------------------------
    def _rediscretise(self, u, adv):
        """Every rank assembles ITS rows only: the level operators become lazy (alfi_amd.lazy.LazyOperator: sparsity now,
        values of a row subset on demand) and DistMultigrid.update cuts the rank's rows out of them -- one rank per mesh
        partition assembling its own cells, as in the reference (alfi/solver.py:604-605).  SUPG terms are assembled by
        the global host pass and keep the replicated path."""
        if self.device_assembly:
            return self._rediscretise_device(u, adv)
        if self.supg:
            self._supg_host_needs_global_values()
            return super()._rediscretise(u, adv)
        if self.burman:
            return self._rediscretise_burman_host(u, adv)
        for L, w in zip(self.levels, self._winds(u)):
            V = L.V
            L.A = LazyOperator(V, L.A.rowptr, L.A.colidx, V.mesh.cell_geometry(), V.element.reference_tensors(), self.nu,
                               self.gamma, adv, np.ascontiguousarray(w), full_div=self.sv)
            L.nu = self.nu
        self._push_operators()

    def _rediscretise_burman_host(self, u, adv):
        """ALFI_DEVICE_ASSEMBLY=0 with Burman terms: every rank assembles its rows on its host cores -- the cells' terms,
        then the host pass over the rank's facets (local_host_operator) -- and hands them and beta_F of its facets (PCPATCH's
        facet rule in the patch factorisation) to its levels."""
        winds = self._winds(u)
        with self._on_stream():
            for dl, LL in zip(self.dmg.levels, self.dmg.local_levels):
                fp = self._facet_parts.get(LL.level)
                if fp is None:            # (ghost copies only: no patch and no product reads those rows)
                    continue
                A, beta = local_host_operator(self.levels[LL.level], LL.part, fp, self.nu, self.gamma, adv, winds[LL.level],
                                              self.burman_weight)
                dl.update_values(A.vals)
                if beta is not None and LL.level > 0:
                    dl.set_facet_beta(beta, adv * self.burman_weight)
        for L in self.levels:
            L.nu = self.nu
        self.dmg.refactor(self.levels)

    def residual(self, u, p, adv):
        """F(u, p) with every rank assembling ITS rows of (nu K + gamma D + 1/2 N(u)) u only -- one pass over its own
        cells instead of two global assemblies on every rank (the replicated host path of the base class, whose cost per
        rank GROWS with the number of ranks sharing the host's cores) -- and the pieces gathered.  SUPG keeps the
        replicated path."""
        if self.device_assembly:
            return self._residual_device(u, p, adv)
        if self.supg:
            self._supg_host_needs_global_values()
            return super().residual(u, p, adv)
        L = self.levels[-1]
        V, d = L.V, L.V.dim
        part = self.dmg.fine.part
        rows = np.asarray(part.own_nodes, dtype=np.int64)
        ptr, cols = _take_rows(L.A.rowptr, L.A.colidx, rows)
        ptr32 = ptr.astype(np.int32)
        g, vol = V.mesh.cell_geometry()
        wind = np.ascontiguousarray(u.reshape(-1, d))
        vals = _hostlib.assemble_bsr(V.cell_nodes, g, vol, V.element.reference_tensors(), d, ptr32, cols, nu=self.nu,
                                     gamma=0.0 if self.sv else self.gamma, gamma_full=self.gamma if self.sv else 0.0,
                                     adv=0.5 * adv, wind=wind if adv else None, row_map=_row_map(V.num_nodes, rows))
        f_own = BSR(len(rows), V.num_nodes, d, ptr32, cols, vals).to_scipy() @ u
        if adv and self.burman:           # + advect * the Burman residual of the rank's rows, over its facets
            fp = self._facet_parts[L.level]
            Fb = np.zeros(part.nb_loc * d)
            fp.host(self.dmg.fine.A, wind[fp.state_nodes], adv * self.burman_weight, F=Fb)
            f_own = f_own + Fb[:part.nb_own * d]
        Fu = np.zeros(self.n_u)
        for dofs, f in self.dmg.comm.all_gather_object((self._own_dofs, f_own)):
            Fu[dofs] = f
        Fu += self.B_raw.T @ p
        if self._load is not None:
            Fu -= self._load
        Fu[L.bc_dofs] = 0.0
        return Fu, self.B_raw @ u

    def _set_parameters(self):
        super()._set_parameters()
        for T in self.transfers:            # (the global transfers follow the rank's)
            T.nu = self.nu

    def _linear_solve(self, rhs):
        sad = self.saddle
        loc = np.concatenate([rhs[:self.n_u][self._own_dofs], rhs[self.n_u:][sad.cells]])
        x, its, rn = sad.solve(loc, self.rtol, self.atol, self.params["ksp_max_it"], 30)
        pieces = self.dmg.comm.all_gather_object((self._own_dofs, sad.cells, x[:sad.n_own], x[sad.n_own:]))
        delta = np.zeros(self.n_u + self.n_p)
        for dofs, cells, xu, xp in pieces:
            delta[dofs] = xu
            delta[self.n_u + np.asarray(cells)] = xp
        return delta, its, rn

    def close(self):
        if getattr(self, "_asm_ready", False):
            self._dB.close()
            self._dBT.close()
            if self._exch is not None:
                self._exch.close()
        self.saddle.close()
        self.dmg.close()
