"""Thin object layer over the C ABI (include/alfi_hip.h): Context, DeviceVec, Level, Transfer, Multigrid.

All arithmetic happens in libalfi_hip.so; this module only moves arrays across the boundary and keeps handles alive.
Errors from the library become ``RuntimeError`` (the reference's plug-ins raise Python exceptions, solver.py:37-38).
"""
import ctypes
import numpy as np

from . import _lib, env
from ._lib import BsrHost, CsrHost, vp


class AlfiHipError(RuntimeError):
    code = None        # the library's error code (ALFI_E_*), where the error came from one of its calls


E_ARG, E_STATE = -2, -3        # ALFI_E_ARG, ALFI_E_STATE


def _ptr(a):
    return None if a is None else a.ctypes.data_as(vp)


class Context(object):
    def __init__(self, device=0, stream=None):
        self.lib = _lib.load()
        h = vp()
        rc = self.lib.alfi_ctx_create(int(device), vp(stream) if stream else None, ctypes.byref(h))
        if rc != 0:
            raise AlfiHipError("alfi_ctx_create failed (%d): %s -- alfi_amd needs an MI355X; there is no CPU fallback"
                               % (rc, self.lib.alfi_last_error(None).decode()))
        self.h = h
        self.device = device

    def check(self, rc):
        if rc != 0:
            e = AlfiHipError("libalfi_hip error %d: %s" % (rc, self.lib.alfi_last_error(self.h).decode()))
            e.code = rc
            raise e

    def sync(self):
        self.check(self.lib.alfi_ctx_sync(self.h))

    def close(self):
        if self.h:
            self.lib.alfi_ctx_destroy(self.h)
            self.h = None

    def set_assembly_scratch(self, max_bytes):
        """Bytes of element blocks the operator refresh may hold at once (alfi_ctx_set_assembly_scratch); beyond, the cells
        are taken in batches."""
        self.check(self.lib.alfi_ctx_set_assembly_scratch(self.h, int(max_bytes)))

    def set_f32_work_bytes(self, n):
        """Cap in bytes on the FP64 work buffer that FP32 levels of big patches are factored through, range by range
        (alfi_ctx_set_f32_work_bytes; default 1 GiB; n <= 0: AlfiHipError with E_ARG)."""
        self.check(self.lib.alfi_ctx_set_f32_work_bytes(self.h, int(n)))

    def f32_work_bytes(self):
        """Bytes of the FP64 work buffer the context holds for its FP32 levels now (alfi_ctx_f32_work_bytes)."""
        b = ctypes.c_int64()
        self.check(self.lib.alfi_ctx_f32_work_bytes(self.h, ctypes.byref(b)))
        return b.value

    def set_condense_min_bytes(self, min_bytes):
        """A level without caller-supplied groups looks for condensable groups in its own sparsity at its first factorisation
        when its dense patch inverses would take at least this many bytes (alfi_ctx_set_condense_min_bytes; default 1 GiB,
        0 = every level, negative = never)."""
        self.check(self.lib.alfi_ctx_set_condense_min_bytes(self.h, int(min_bytes)))

    def set_comm(self, callback, dred_ptr, dred_len):
        """callback: a ctypes function pointer of type alfi_amd.dist.CommFn (kept alive by the caller)."""
        self.check(self.lib.alfi_ctx_set_comm(self.h, ctypes.cast(callback, vp), None, vp(int(dred_ptr)), int(dred_len)))

    def comm_init(self, unique_id, rank, nranks):
        """Native transport: the ctx creates its own RCCL communicator from the 128-byte id (collective over the ranks)."""
        buf = ctypes.create_string_buffer(bytes(unique_id), _lib.COMM_ID_BYTES)
        self.check(self.lib.alfi_ctx_comm_init(self.h, ctypes.cast(buf, vp), int(rank), int(nranks)))

    def comm_allow_self(self, on=True):
        """TEST HOOK (alfi_ctx_comm_allow_self): a rank may name itself as a neighbour."""
        self.check(self.lib.alfi_ctx_comm_allow_self(self.h, 1 if on else 0))

    def comm_size(self):
        """(rank, ranks) of the communicator the library itself exchanges over (alfi_ctx_comm_size)."""
        r, n = ctypes.c_int(), ctypes.c_int()
        self.check(self.lib.alfi_ctx_comm_size(self.h, ctypes.byref(r), ctypes.byref(n)))
        return r.value, n.value

    # vectors ----------------------------------------------------------------------------------------------------------
    def vec(self, n_or_array):
        if isinstance(n_or_array, (int, np.integer)):
            v = DeviceVec(self, int(n_or_array))
            v.zero()
            return v
        a = np.ascontiguousarray(n_or_array, dtype=np.float64)
        v = DeviceVec(self, a.shape[0])
        v.set(a)
        return v

    def mat(self, n_or_array, ncol=None, ld=None):
        """A block operand (DeviceMat): ``mat(n, ncol)`` zeroed, or ``mat(array)`` from an (n, ncol) array, one column per
        right-hand side; ``ld``: its leading dimension (default: n rounded up to even)."""
        if isinstance(n_or_array, (int, np.integer)):
            return DeviceMat(self, int(n_or_array), int(ncol), ld)
        a = np.asarray(n_or_array, dtype=np.float64)
        if a.ndim != 2:
            raise ValueError("a block operand is an (n, ncol) array")
        m = DeviceMat(self, a.shape[0], a.shape[1], ld)
        m.set(a)
        return m

    def set_block_kernels(self, on=True):
        """Block calls take the batched kernels where a level has them (alfi_ctx_set_block_kernels; default on).  Off: every
        block call loops the single-vector call over its columns -- the same bits at the cost of ncol single calls."""
        self.check(self.lib.alfi_ctx_set_block_kernels(self.h, 1 if on else 0))

    def set_block_fused(self, on=True):
        """The block smoother takes the block form of the four-launch iteration on the levels that have it
        (alfi_ctx_set_block_fused; default on; ``Level.smooth_block_mode`` says which).  Off: those levels loop whole smoother
        calls over the columns while every other block kernel stays on -- the same bits; the A/B switch of that form."""
        self.check(self.lib.alfi_ctx_set_block_fused(self.h, 1 if on else 0))

    def set_block_lds_bytes(self, nbytes=64 * 1024):
        """LDS a workgroup of a block apply may ask for (alfi_ctx_set_block_lds_bytes; default 64 KiB, clamped to the device's
        limit per workgroup).  One budget for both applies that batch by it: a condensed level batches the widest NV of 4, 3, 2
        with NV x the LDS of its one-vector kernels within it, a level of dense macro-star inverses (a patch above 160 dofs) the
        widest NV with NV x 8 x (its largest patch, rounded up to even) bytes within it -- 4 columns up to 2048 dofs at the
        default, 3 up to 2730, 2 up to 4096 (``Level.patch_apply_block_width``).  The de-duplicated level product batches by it
        too: the widest NV with NV x 8 x bs x (the largest number of distinct columns in a group of 1024 blocks) bytes within it --
        at the default bs 2 always 4, bs 3 4 columns up to 682 distinct columns, 3 up to 910, 2 up to 1024
        (``Level.spmv_block_width``).  The A/B and test switch of those widths; never the bits."""
        self.check(self.lib.alfi_ctx_set_block_lds_bytes(self.h, int(nbytes)))

    # profiling (PETSc-event style report, driver.py:77-92) ----------------------------------------------------------------
    def transfer_stats(self, reset=False):
        """(bytes host -> device, bytes device -> host) of every copy the library made since the last reset, process-wide
        (alfi_transfer_stats)."""
        a, b = ctypes.c_int64(), ctypes.c_int64()
        self.check(self.lib.alfi_transfer_stats(ctypes.byref(a), ctypes.byref(b), 1 if reset else 0))
        return a.value, b.value

    def axpy(self, y, x, a, n=None, y_off=0, x_off=0):
        """y[y_off : y_off + n] += a x[x_off : x_off + n] on the device (alfi_vec_axpy)."""
        n = min(y.n - y_off, x.n - x_off) if n is None else int(n)
        self.check(self.lib.alfi_vec_axpy(self.h, vp(y.ptr.value + 8 * y_off), vp(x.ptr.value + 8 * x_off), float(a), n))

    def copy(self, y, x, n=None, y_off=0, x_off=0):
        """y[y_off : y_off + n] = x[x_off : x_off + n] on the device (alfi_vec_copy)."""
        n = min(y.n - y_off, x.n - x_off) if n is None else int(n)
        self.check(self.lib.alfi_vec_copy(self.h, vp(y.ptr.value + 8 * y_off), vp(x.ptr.value + 8 * x_off), n))

    def ivec(self, a):
        """A device array of int32 (index lists of alfi_vec_gather)."""
        return IntVec(self, a)

    def gather(self, dst, src, idx, bs=1):
        """dst[i] = src[idx[i]], bs consecutive doubles per index, on the device (alfi_vec_gather; idx: an IntVec)."""
        assert dst.n >= idx.n * bs
        self.check(self.lib.alfi_vec_gather(self.h, dst.ptr, src.ptr, idx.ptr, idx.n, int(bs)))

    def gather_csr(self, dst, src, rowptr, colidx, weights, bs=1):
        """dst[i*bs + c] = sum_k weights[k] * src[colidx[k]*bs + c] over CSR row i, on the device (alfi_vec_gather_csr; rowptr,
        colidx: IntVecs, weights: a device vector; bs 1, 2 or 3)."""
        nrows = rowptr.n - 1
        assert nrows >= 0 and dst.n >= nrows * bs and colidx.n <= weights.n
        self.check(self.lib.alfi_vec_gather_csr(self.h, dst.ptr, src.ptr, rowptr.ptr, colidx.ptr, weights.ptr, nrows, int(bs)))

    def comm_stats(self, reset=False):
        """(halo exchanges, all-reduces, doubles sent by this rank) since the last reset (alfi_ctx_comm_stats)."""
        a, b, c = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        self.check(self.lib.alfi_ctx_comm_stats(self.h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), 1 if reset else 0))
        return a.value, b.value, c.value

    def set_graph(self, on=True):
        """Replay whole multigrid cycles as hipGraphs (alfi_ctx_set_graph)."""
        self.check(self.lib.alfi_ctx_set_graph(self.h, 1 if on else 0))

    def prof_enable(self, on=True):
        """True / 1: every event class; 2: PATCH_APPLY and COMM only; False / 0: off."""
        self.check(self.lib.alfi_prof_enable(self.h, int(on)))

    def prof_reset(self):
        self.check(self.lib.alfi_prof_reset(self.h))

    def prof_get(self, level_id=-1, petsc_names=False):
        """{event name: (total device ms, launches)} since the last reset, optionally for one level only; ``petsc_names``: keyed
        by the PETSc log events of the reference's report (alfi/driver.py:80) instead of the library's class names."""
        out = {}
        for i, name in enumerate(_lib.EVENTS):
            ms, cnt = ctypes.c_double(), ctypes.c_int64()
            self.check(self.lib.alfi_prof_get_level(self.h, i, int(level_id), ctypes.byref(ms), ctypes.byref(cnt)))
            out[_lib.PETSC_EVENT_NAMES[name] if petsc_names else name] = (ms.value, cnt.value)
        return out


class DeviceVec(object):
    """A level vector resident in HBM (the analogue of a PETSc Vec's local array)."""

    def __init__(self, ctx, n):
        self.ctx, self.n = ctx, int(n)
        p = vp()
        ctx.check(ctx.lib.alfi_malloc(ctx.h, self.n * 8, ctypes.byref(p)))
        self.ptr = p

    def set(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        assert a.shape == (self.n,)
        self.ctx.check(self.ctx.lib.alfi_memcpy_h2d(self.ctx.h, self.ptr, _ptr(a), self.n * 8))

    def get(self):
        out = np.empty(self.n, dtype=np.float64)
        self.ctx.check(self.ctx.lib.alfi_memcpy_d2h(self.ctx.h, _ptr(out), self.ptr, self.n * 8))
        return out

    def zero(self):
        self.ctx.check(self.ctx.lib.alfi_memset0(self.ctx.h, self.ptr, self.n * 8))

    def __del__(self):
        try:
            if self.ptr and self.ctx.h:
                self.ctx.lib.alfi_free(self.ctx.h, self.ptr)
        except Exception:
            pass
        self.ptr = None


class DeviceMat(object):
    """A block operand of the ``*_block`` calls: ncol right-hand sides as the columns of a column-major device matrix, column c
    at ``ptr + 8 c ld`` (``ld`` >= n and even, so that every column is 16-byte aligned).  The entries between n and ld are never
    read or written by the library."""

    def __init__(self, ctx, n, ncol, ld=None):
        self.ctx, self.n, self.ncol = ctx, int(n), int(ncol)
        self.ld = (self.n + 1) & ~1 if ld is None else int(ld)
        if self.ncol < 1 or self.ld < self.n or self.ld & 1:
            raise ValueError("a block operand needs ncol >= 1 and an even leading dimension >= n (n %d, ncol %d, ld %d)"
                             % (self.n, self.ncol, self.ld))
        self._buf = DeviceVec(ctx, max(self.ld * self.ncol, 1))
        self._buf.zero()
        self.ptr = self._buf.ptr

    def set(self, a):
        a = np.asarray(a, dtype=np.float64)
        assert a.shape == (self.n, self.ncol), (a.shape, self.n, self.ncol)
        h = np.zeros((self.ncol, self.ld))
        h[:, :self.n] = a.T
        self._buf.set(h.ravel())

    def get(self):
        """The (n, ncol) array."""
        return np.ascontiguousarray(self._buf.get().reshape(self.ncol, self.ld)[:, :self.n].T)

    def col(self, c):
        """Column c as a device vector (no copy)."""
        assert 0 <= c < self.ncol
        return view(self._buf, c * self.ld, self.n)

    def zero(self):
        self._buf.zero()


def _block_args(n, cols, *mats):
    """(ncol, cols pointer, nx, kept array) of a block call on the DeviceMats ``mats`` of n-vectors; cols None: every column."""
    nx = mats[0].ncol
    for m in mats:
        if m.n != n or m.ncol != nx:
            raise ValueError("block operands of %d columns of length %d expected, got %d of length %d" % (nx, n, m.ncol, m.n))
    if cols is None:
        return nx, None, nx, None
    c = np.ascontiguousarray(cols, dtype=np.int32)
    return len(c), _ptr(c), nx, c


class IntVec(object):
    """int32 indices resident on the device."""

    def __init__(self, ctx, a):
        a = np.ascontiguousarray(a, dtype=np.int32)
        self.ctx, self.n = ctx, int(a.shape[0])
        p = vp()
        ctx.check(ctx.lib.alfi_malloc(ctx.h, max(self.n, 1) * 4, ctypes.byref(p)))
        self.ptr = p
        if self.n:
            ctx.check(ctx.lib.alfi_memcpy_h2d(ctx.h, p, _ptr(a), self.n * 4))

    def __del__(self):
        try:
            if self.ptr and self.ctx.h:
                self.ctx.lib.alfi_free(self.ctx.h, self.ptr)
        except Exception:
            pass
        self.ptr = None


def _bsr_struct(B, keep):
    rowptr = np.ascontiguousarray(B.rowptr, dtype=np.int32)
    colidx = np.ascontiguousarray(B.colidx, dtype=np.int32)
    vals = np.ascontiguousarray(B.vals, dtype=np.float64)
    keep.extend([rowptr, colidx, vals])
    return BsrHost(B.nbrows, B.nbcols, _ptr(rowptr), _ptr(colidx), _ptr(vals))


class Level(object):
    """One multigrid level: BSR operator + Dirichlet dofs (+ patches)."""

    def __init__(self, ctx, A, bc_dofs):
        self.ctx = ctx
        self.n, self.bs = A.nbrows * A.bs, A.bs
        bc = np.ascontiguousarray(bc_dofs, dtype=np.int32)
        h = vp()
        # (A.vals None: the sparsity only, the values are formed on the device -- set_assembly + assemble)
        vals = None if A.vals is None else np.ascontiguousarray(A.vals)
        ctx.check(ctx.lib.alfi_level_create(ctx.h, A.nbrows, A.bs, _ptr(A.rowptr), _ptr(A.colidx), _ptr(vals), _ptr(bc), len(bc),
                                            ctypes.byref(h)))
        self.h = h
        self.nnzb = A.nnzb
        i = ctypes.c_int()
        ctx.check(ctx.lib.alfi_level_id(h, ctypes.byref(i)))
        self.id = i.value

    def set_partition(self, nb_owned, distributed, send_nodes, sendbuf_ptr, recvbuf_ptr, nb_ghost):
        """sendbuf_ptr / recvbuf_ptr: device buffers the callback transport exchanges, or None: library-owned."""
        sn = np.ascontiguousarray(send_nodes, dtype=np.int32)
        sp_, rp_ = (vp(int(sendbuf_ptr)), vp(int(recvbuf_ptr))) if sendbuf_ptr is not None else (None, None)
        self.ctx.check(self.ctx.lib.alfi_level_set_partition(self.h, int(nb_owned), 1 if distributed else 0, len(sn),
                                                             _ptr(sn), sp_, rp_, int(nb_ghost)))
        self.n_own = int(nb_owned) * self.bs

    def set_sum_exchange(self, ranks, counts, send_nodes, sum_nodes, sum_ptr, sum_src):
        """Plan of the merged reverse-add + forward exchange of the smoother (alfi_level_set_sum_exchange, native transport)."""
        ranks = np.ascontiguousarray(ranks, dtype=np.int32)
        counts = np.ascontiguousarray(counts, dtype=np.int64)
        send_nodes = np.ascontiguousarray(send_nodes, dtype=np.int32)
        sum_nodes = np.ascontiguousarray(sum_nodes, dtype=np.int32)
        sum_ptr = np.ascontiguousarray(sum_ptr, dtype=np.int32)
        sum_src = np.ascontiguousarray(sum_src, dtype=np.int32)
        assert send_nodes.shape[0] == counts.sum() and sum_ptr.shape[0] == sum_nodes.shape[0] + 1
        self.ctx.check(self.ctx.lib.alfi_level_set_sum_exchange(self.h, len(ranks), _ptr(ranks), _ptr(counts), _ptr(send_nodes),
                                                                len(sum_nodes), _ptr(sum_nodes), _ptr(sum_ptr), _ptr(sum_src)))

    def set_neighbours(self, ranks, send_nodes, recv_nodes):
        """Native transport: neighbour ranks (ascending) and the nodes sent to / received from each."""
        r = np.ascontiguousarray(ranks, dtype=np.int32)
        sc = np.ascontiguousarray(send_nodes, dtype=np.int64)
        rc = np.ascontiguousarray(recv_nodes, dtype=np.int64)
        self.ctx.check(self.ctx.lib.alfi_level_set_neighbours(self.h, len(r), _ptr(r), _ptr(sc), _ptr(rc)))

    def set_overlap(self, nb_interior, npatch_interior):
        self.ctx.check(self.ctx.lib.alfi_level_set_overlap(self.h, int(nb_interior), int(npatch_interior)))

    def update_values(self, vals):
        vals = np.ascontiguousarray(vals, dtype=np.float64)
        self.ctx.check(self.ctx.lib.alfi_level_update_values(self.h, _ptr(vals)))

    def set_assembly(self, V, rowptr, colidx, full_div=False, cells=None, cell_nodes=None):
        """Hand the level what the device-side operator refresh needs (alfi_level_set_assembly): the cells of the nodal
        space ``V`` (alfi_amd.fespace), the reference-cell tensors of its element (viscous / grad-div / advection terms) and
        the contributor lists of the level's sparsity; ``full_div``: the Scott-Vogelius grad-div term (solver.py:616).
        Partitioned level (alfi_amd.dist): ``cells`` = the mesh cells that touch a local node, ``cell_nodes`` their nodes in
        the numbering of the rank's state vector (local nodes first, then the cells' other nodes); rowptr / colidx the LOCAL
        operator's."""
        from . import _hostlib
        g, vol = V.mesh.cell_geometry()
        tens = V.element.reference_tensors()
        S, bI, T1 = (np.ascontiguousarray(tens[k], dtype=np.float64) for k in ("S", "bI", "T1"))
        nrows = len(rowptr) - 1
        if cells is None:
            cn = np.ascontiguousarray(V.cell_nodes, dtype=np.int32)
            cptr, ccell, cba = _hostlib.contributors(cn, V.num_nodes, rowptr, colidx)
        else:
            cn = np.ascontiguousarray(cell_nodes, dtype=np.int32)
            g, vol = g[cells], vol[cells]
            cptr, ccell, cba = _hostlib.contributors(cn, nrows, rowptr, colidx, nindex=int(cn.max()) + 1 if cn.size else nrows,
                                                     partial=True)
        g = np.ascontiguousarray(g, dtype=np.float64)
        vol = np.ascontiguousarray(vol, dtype=np.float64)
        self.ctx.check(self.ctx.lib.alfi_level_set_assembly(self.h, cn.shape[0], cn.shape[1], _ptr(cn), _ptr(g), _ptr(vol),
                                                            _ptr(S), _ptr(bI), _ptr(T1), 1 if full_div else 0, _ptr(cptr),
                                                            _ptr(ccell), _ptr(cba)))

    def set_assembly_bc(self, bc_dofs):
        """Partitioned level: the Dirichlet dofs among ALL local dofs, ghosts included (alfi_level_set_assembly_bc)."""
        b = np.ascontiguousarray(bc_dofs, dtype=np.int32)
        self.ctx.check(self.ctx.lib.alfi_level_set_assembly_bc(self.h, _ptr(b), b.shape[0]))

    def assembly_state_size(self):
        n = ctypes.c_int64()
        self.ctx.check(self.ctx.lib.alfi_level_assembly_state_size(self.h, ctypes.byref(n)))
        return n.value

    def assemble_mult(self, nu, gamma, adv, state, x, y):
        """y = (nu K + gamma D + adv N(state)) x without boundary conditions, matrix-free (alfi_level_assemble_mult): the
        level's operator and patch factors stay as they are."""
        self.ctx.check(self.ctx.lib.alfi_level_assemble_mult(self.h, float(nu), float(gamma), float(adv),
                                                             state.ptr if state is not None else None, x.ptr, y.ptr))

    def set_supg(self, V, nq=None, cells=None):
        """Quadrature tables for the device-side SUPG terms (alfi_level_set_supg): the rule and tabulation of
        ``_hostlib.supg`` (degree 2k) and the cell sizes.  ``cells`` (partitioned level): the cells given to
        ``set_assembly``."""
        from . import _hostlib
        el = V.element
        lam, wq = _hostlib.supg_rule(V, nq)
        phi, dphi = el.tabulate(lam)
        d2phi = el.tabulate_hessian(lam)
        h = _hostlib.cell_size(V.mesh)
        if cells is not None:
            h = np.asarray(h)[np.asarray(cells)]
        arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (wq, phi, dphi, d2phi, h)]
        self.ctx.check(self.ctx.lib.alfi_level_set_supg(self.h, len(wq), _ptr(arrs[0]), _ptr(arrs[1]), _ptr(arrs[2]),
                                                        _ptr(arrs[3]), _ptr(arrs[4])))

    def assemble_supg(self, nu, gamma, adv, state, weight, magic, apply_bc=True):
        """The refresh of a stabilised run in one pass (alfi_level_assemble_supg): A = nu K + gamma D + adv N(state) + the
        linearised SUPG term, then the boundary conditions."""
        self.ctx.check(self.ctx.lib.alfi_level_assemble_supg(self.h, float(nu), float(gamma), float(adv), state.ptr,
                                                             float(weight), float(magic), 1 if apply_bc else 0))

    def set_supg_load(self, fq):
        """The body force at the points of ``set_supg``'s rule, (ncell, nq, dim) -- see ``supg_load`` --, subtracted in the
        strong residual of the SUPG and GLS terms (alfi_level_set_supg_load); None removes it."""
        if fq is None:
            self.ctx.check(self.ctx.lib.alfi_level_set_supg_load(self.h, None))
            return
        f = np.ascontiguousarray(fq, dtype=np.float64)
        self.ctx.check(self.ctx.lib.alfi_level_set_supg_load(self.h, _ptr(f)))

    def assemble_gls(self, nu, gamma, adv, state, wind, weight, magic, apply_bc=True):
        """The refresh of a GLS-stabilised run in one pass (alfi_level_assemble_gls): A = nu K + gamma D + adv N(state) + the
        linearised GLS term about ``state`` with the wind ``wind`` (device vectors), then the boundary conditions."""
        self.ctx.check(self.ctx.lib.alfi_level_assemble_gls(self.h, float(nu), float(gamma), float(adv), state.ptr, wind.ptr,
                                                            float(weight), float(magic), 1 if apply_bc else 0))

    def gls(self, nu, weight, magic, state, wind, add_to_operator=True, F=None):
        """GLS terms about ``state`` with the wind ``wind`` on the device (alfi_level_gls): the linearisation into the operator
        and / or the residual contribution added to the device vector ``F``."""
        self.ctx.check(self.ctx.lib.alfi_level_gls(self.h, float(nu), float(weight), float(magic), state.ptr, wind.ptr,
                                                   1 if add_to_operator else 0, F.ptr if F is not None else None))

    def supg(self, nu, weight, magic, state, add_to_operator=True, F=None):
        """SUPG terms about ``state`` on the device (alfi_level_supg): the linearisation into the operator and / or the
        residual contribution added to the device vector ``F``."""
        self.ctx.check(self.ctx.lib.alfi_level_supg(self.h, float(nu), float(weight), float(magic), state.ptr,
                                                    1 if add_to_operator else 0, F.ptr if F is not None else None))

    def apply_bc(self):
        self.ctx.check(self.ctx.lib.alfi_level_apply_bc(self.h))

    def set_facet_blocks(self, on=True):
        """The level's sparsity couples the nodes of cells that share a facet (alfi_level_set_facet_blocks; before
        ``set_assembly``): blocks without a contributing cell are accepted."""
        self.ctx.check(self.ctx.lib.alfi_level_set_facet_blocks(self.h, 1 if on else 0))

    def set_burman(self, table, rowptr, colidx, lists=None):
        """Interior-facet tables and contributor lists of the Burman term (alfi_level_set_burman); ``table``:
        burman.FacetTable of the level, rowptr / colidx: the level's (facet-coupled) sparsity.  lists: the contributor lists
        if the caller has them (a partitioned level: alfi_amd.dist.FacetPart.lists)."""
        t = table
        (bptr, bfac, bab), (nptr, nfac, na) = lists if lists is not None else t.contributors(rowptr, colidx, len(rowptr) - 1)
        f64 = [np.ascontiguousarray(a, dtype=np.float64) for a in (t.J, t.area, t.coef, t.ws, t.wn, t.phin)]
        i32 = [np.ascontiguousarray(a, dtype=np.int32) for a in (t.union, t.cfg, bfac, nfac)]
        i64 = [np.ascontiguousarray(a, dtype=np.int64) for a in (bptr, nptr)]
        u16 = [np.ascontiguousarray(a, dtype=np.uint16) for a in (bab, na)]
        self.ctx.check(self.ctx.lib.alfi_level_set_burman(
            self.h, int(t.nf), int(t.nu), len(t.ws), len(t.wn), int(t.phin.shape[0]), _ptr(i32[0]), _ptr(i32[1]), _ptr(f64[0]),
            _ptr(f64[1]), _ptr(f64[2]), _ptr(f64[3]), _ptr(f64[4]), _ptr(f64[5]), _ptr(i64[0]), _ptr(i32[2]), _ptr(u16[0]),
            _ptr(i64[1]), _ptr(i32[3]), _ptr(u16[1])))

    def burman(self, weight, state, add_to_operator=True, F=None):
        """Burman terms about ``state`` on the device (alfi_level_burman): ``weight`` times the linearisation into the
        operator and / or the residual contribution added to the device vector ``F``."""
        self.ctx.check(self.ctx.lib.alfi_level_burman(self.h, float(weight), state.ptr, 1 if add_to_operator else 0,
                                                      F.ptr if F is not None else None))

    def set_patch_facet_correction(self, nfacet, ptr, col, fac, s):
        """PCPATCH's facet rule on a Burman level (alfi_patches_set_facet_correction): burman.patch_facet_corrections."""
        ptr = np.ascontiguousarray(ptr, dtype=np.int64)
        col, fac = (np.ascontiguousarray(a, dtype=np.int32) for a in (col, fac))
        s = np.ascontiguousarray(s, dtype=np.float64)
        self.ctx.check(self.ctx.lib.alfi_patches_set_facet_correction(self.h, int(nfacet), len(ptr) - 1, _ptr(ptr), _ptr(col),
                                                                      _ptr(fac), _ptr(s)))
        self._record_storage()

    def set_facet_beta(self, beta, scale):
        """beta_F of every facet and adv * weight of host-assembled operator values (alfi_level_set_facet_beta)."""
        beta = np.ascontiguousarray(beta, dtype=np.float64)
        self.ctx.check(self.ctx.lib.alfi_level_set_facet_beta(self.h, _ptr(beta), float(scale)))

    def assemble_burman(self, nu, gamma, adv, state, weight, apply_bc=True):
        """The refresh of a Burman-stabilised run (alfi_level_assemble_burman): A = nu K + gamma D + adv N(state) + adv *
        weight * the linearised Burman term, then the boundary conditions."""
        self.ctx.check(self.ctx.lib.alfi_level_assemble_burman(self.h, float(nu), float(gamma), float(adv), state.ptr,
                                                               float(weight), 1 if apply_bc else 0))

    def assemble(self, nu, gamma, adv, state=None, apply_bc=True):
        """A = nu K + gamma D + adv N(state) written into the level's operator on the device (alfi_level_assemble);
        ``state``: DeviceVec / RawVec with the level's nodal field.  The patches must be factored again afterwards."""
        self.ctx.check(self.ctx.lib.alfi_level_assemble(self.h, float(nu), float(gamma), float(adv),
                                                        state.ptr if state is not None else None, 1 if apply_bc else 0))

    def transpose(self):
        """The operator replaced by its block transpose on the device, in the same sparsity and bitwise (alfi_level_transpose:
        the velocity block of the adjoint J^T).  Serial levels with a structurally symmetric pattern only (a partitioned level
        refreshes A^T instead: ``set_assembly_transposed``); the patches and the coarse grid must be factored again afterwards."""
        self.ctx.check(self.ctx.lib.alfi_level_transpose(self.h))

    def set_assembly_transposed(self, on=True):
        """While on, every device refresh of this level (``assemble`` / ``assemble_supg`` / ``assemble_gls`` /
        ``assemble_burman`` and ``supg`` / ``gls`` / ``burman`` adding to the operator) writes A^T in the same sparsity, bitwise
        what a refresh followed by ``transpose`` gives (alfi_level_set_assembly_transposed).  Serial and partitioned levels,
        after ``set_assembly``; ``assemble_mult`` and the residual outputs stay forward quantities."""
        self.ctx.check(self.ctx.lib.alfi_level_set_assembly_transposed(self.h, 1 if on else 0))

    def get_values(self):
        """The operator values in the host layout (nnzb, bs, bs)."""
        out = np.empty((self.nnzb, self.bs, self.bs))
        self.ctx.check(self.ctx.lib.alfi_level_get_values(self.h, _ptr(out)))
        return out

    def set_patches(self, patch_ptr, patch_dofs):
        pp = np.ascontiguousarray(patch_ptr, dtype=np.int64)
        pd = np.ascontiguousarray(patch_dofs, dtype=np.int32)
        self.ctx.check(self.ctx.lib.alfi_patches_set(self.h, len(pp) - 1, _ptr(pp), _ptr(pd)))

    def set_patch_groups(self, groups):
        """Condensed patch factors (alfi_patches_set_groups): one label per entry of patch_dofs, >= 0 = group of the patch the
        entry belongs to, -1 = skeleton; None = dense inverses."""
        g = None if groups is None else np.ascontiguousarray(groups, dtype=np.int32)
        self.ctx.check(self.ctx.lib.alfi_patches_set_groups(self.h, _ptr(g)))
        self._record_storage()

    host_level = None      # the host level these patches belong to (note_patch_level)

    def _record_storage(self):
        if self.host_level is not None and self.h:
            self.host_level.patch_storage = self.condensed()
            self.host_level.patch_factor_bytes = self.factor_bytes()
            self.host_level.patch_factor_dtype = self.patch_storage_dtype()

    STORAGE_DTYPES = {"f64": 0, "f32": 1}          # ALFI_STORAGE_F64 / ALFI_STORAGE_F32

    def set_patch_storage(self, dtype):
        """Storage of the level's dense patch inverses from its next ``factor()`` on (alfi_patches_set_storage): "f64" or "f32"
        -- single precision in device memory, every product and sum of the apply still FP64.  AlfiHipError with ``code ==
        E_ARG`` where no FP32 form exists (small 2-D stars, macro stars, caller-supplied groups, multiplicative sweeps, a facet
        correction); the level stays as it was."""
        if dtype not in self.STORAGE_DTYPES:
            raise ValueError("patch storage %r (f64 or f32)" % (dtype,))
        self.ctx.check(self.ctx.lib.alfi_patches_set_storage(self.h, self.STORAGE_DTYPES[dtype]))

    def set_macro_patch_storage(self, dtype):
        """The FP32 request of macro stars and Burman levels (alfi_patches_set_macro_storage): "f64" or "f32" from the next
        ``factor()`` on.  Accepts what ``set_patch_storage`` refuses -- a patch above 160 dofs (the level is then factored in
        patch ranges through the context's work buffer, ``Context.set_f32_work_bytes``) and a facet correction, set before or
        after.  AlfiHipError with ``code == E_ARG`` where no FP32 form exists (no patches, every patch <= 32 dofs,
        caller-supplied groups, multiplicative sweeps); the level stays as it was."""
        if dtype not in self.STORAGE_DTYPES:
            raise ValueError("patch storage %r (f64 or f32)" % (dtype,))
        self.ctx.check(self.ctx.lib.alfi_patches_set_macro_storage(self.h, self.STORAGE_DTYPES[dtype]))

    def set_patch_canonical_order(self, rank):
        """FP32 levels (alfi_patches_set_canonical_order): ``rank[q]`` = the place of entry q of patch_dofs in a canonical
        order of its patch -- for a rank's local level the order of the unpartitioned patch (dist.localize_level: ``patch_rank``),
        so that the stored float32 values do not depend on the partition; None: the order of patch_dofs."""
        r = None if rank is None else np.ascontiguousarray(rank, dtype=np.int32)
        self.ctx.check(self.ctx.lib.alfi_patches_set_canonical_order(self.h, _ptr(r)))

    def patch_storage_dtype(self):
        """"f64" or "f32": what the level holds now (alfi_patches_storage; a request takes effect at the next ``factor()``)."""
        d = ctypes.c_int()
        self.ctx.check(self.ctx.lib.alfi_patches_storage(self.h, ctypes.byref(d)))
        return "f32" if d.value == 1 else "f64"

    def find_patch_groups(self):
        """Group labels found from the level's block sparsity (alfi_patches_find_groups): one per entry of patch_dofs, -1 =
        skeleton; what the level uses by itself when its dense inverses would be large (Context.set_condense_min_bytes)."""
        a, b, c = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        self.ctx.check(self.ctx.lib.alfi_patches_stats(self.h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        g = np.empty(b.value, dtype=np.int32)
        self.ctx.check(self.ctx.lib.alfi_patches_find_groups(self.h, _ptr(g)))
        return g

    def condensed(self):
        """0: dense inverses, 1: condensed factors on the caller's groups, 2: on groups the library found itself
        (alfi_patches_condensed; final after the first ``factor()`` of a patch set)."""
        m = ctypes.c_int()
        self.ctx.check(self.ctx.lib.alfi_patches_condensed(self.h, ctypes.byref(m)))
        return m.value

    def factor_bytes(self):
        b = ctypes.c_int64()
        self.ctx.check(self.ctx.lib.alfi_patches_factor_bytes(self.h, ctypes.byref(b)))
        return b.value

    def set_partition_of_unity(self, on=True):
        self.ctx.check(self.ctx.lib.alfi_patches_set_partition_of_unity(self.h, 1 if on else 0))

    def set_multiplicative(self, iterset, symmetrise, condensed=False):
        """Multiplicative sweeps in the order ``iterset`` (None / empty = back to additive); returns the number of
        dependency wavefronts one sweep was scheduled into.  ``condensed``: a level with the caller's groups
        (``set_patch_groups``) keeps its condensed factors and sweeps over them (alfi_patches_set_multiplicative_condensed);
        on any other level the flag changes nothing."""
        it = np.ascontiguousarray(iterset if iterset is not None else [], dtype=np.int64)
        fn = self.ctx.lib.alfi_patches_set_multiplicative_condensed if condensed else self.ctx.lib.alfi_patches_set_multiplicative
        self.ctx.check(fn(self.h, len(it), _ptr(it), 1 if symmetrise else 0))
        self._record_storage()
        nw = ctypes.c_int64()
        self.ctx.check(self.ctx.lib.alfi_patches_multiplicative_levels(self.h, ctypes.byref(nw)))
        return nw.value

    def factor(self):
        self.ctx.check(self.ctx.lib.alfi_patches_factor(self.h))
        self._record_storage()

    def factor_with_fallback(self):
        """factor(); condensed factors that fail the residual probe are repaired in place (pivoted LU of their Schur
        complements, kernels_check.hip).  Only if they STILL fail beyond ALFI_PATCH_CHECK_FAIL -- or the repair does not
        apply (Schur complements above 4096 dofs) -- fall back to dense inverses for this level and factor again.  Returns
        True if it fell back."""
        try:
            self.factor()
            self._warn_if_flagged()
            return False
        except AlfiHipError as e:
            if "condensed" not in str(e):
                raise
        self.set_patch_groups(None)
        self.factor()
        self._warn_if_flagged()
        return True

    def _warn_if_flagged(self):
        """the setup only FAILS beyond 1000 x the probe tolerance; patches that stay above the tolerance after the
        pivoted repair (ill-conditioned, not mis-factored: LAPACK would return the same inverse) degrade the smoother
        silently unless somebody says so."""
        worst, flagged, repaired, after = self.patch_check()
        if flagged > repaired:
            import warnings
            warnings.warn("alfi_patches_factor: %d of %d flagged patch factors stay above the probe tolerance after the "
                          "pivoted repair (worst residual %.2e): the patch operators are ill-conditioned"
                          % (flagged - repaired, flagged, after))

    def patch_check(self):
        """(worst residual || A_p X_p e - e || of the fast inversion, patches flagged, patches repaired by the pivoted
        re-inversion, worst residual afterwards) of the last ``factor()``."""
        w, wa = ctypes.c_double(), ctypes.c_double()
        f, r = ctypes.c_int64(), ctypes.c_int64()
        self.ctx.check(self.ctx.lib.alfi_patches_check(self.h, ctypes.byref(w), ctypes.byref(f), ctypes.byref(r),
                                                       ctypes.byref(wa)))
        return w.value, f.value, r.value, wa.value

    def patch_stats(self):
        a, b, c = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        self.ctx.check(self.ctx.lib.alfi_patches_stats(self.h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return a.value, b.value, c.value

    def patch_inverse(self, p, n):
        out = np.empty((n, n))
        self.ctx.check(self.ctx.lib.alfi_patch_get_inverse(self.h, int(p), _ptr(out)))
        return out

    def patch_apply(self, x, y):
        self.ctx.check(self.ctx.lib.alfi_patch_apply(self.h, x.ptr, y.ptr))

    def patch_apply_split(self, split, x, y):
        """TEST HOOK (alfi_patch_apply_split): the additive apply as the range launches [0, split) and [split, npatch)."""
        self.ctx.check(self.ctx.lib.alfi_patch_apply_split(self.h, int(split), x.ptr, y.ptr))

    def spmv(self, x, y):
        self.ctx.check(self.ctx.lib.alfi_spmv(self.h, x.ptr, y.ptr))

    def zero_bc(self, v):
        """v[Dirichlet dofs of the level] = 0 on the device (alfi_level_zero_bc)."""
        self.ctx.check(self.ctx.lib.alfi_level_zero_bc(self.h, v.ptr))

    def halo_forward(self, v):
        """Partitioned level: ghost slots of v <- their owners' values (no-op otherwise)."""
        self.ctx.check(self.ctx.lib.alfi_level_halo_forward(self.h, v.ptr))

    def halo_sum(self, v):
        """Partitioned level with a sum-exchange plan: every holder of a shared node gets the sum of all holders' values."""
        self.ctx.check(self.ctx.lib.alfi_level_halo_sum(self.h, v.ptr))

    def halo_reverse_add(self, v):
        """Partitioned level: ghost slots of v added onto their owners' entries (no-op otherwise)."""
        self.ctx.check(self.ctx.lib.alfi_level_halo_reverse_add(self.h, v.ptr))

    def residual(self, b, x, r):
        self.ctx.check(self.ctx.lib.alfi_residual(self.h, b.ptr, x.ptr, r.ptr))

    def smooth(self, k, b, x, nonzero_guess=True):
        self.ctx.check(self.ctx.lib.alfi_smooth_fgmres(self.h, int(k), b.ptr, x.ptr, 1 if nonzero_guess else 0))

    # block right-hand sides (DeviceMat operands; cols: the columns to work on, None = all) -- column c of every result is the
    # single-vector call on column c bit for bit
    def patch_apply_block(self, X, Y, cols=None):
        ncol, cp, nx, keep = _block_args(self.n, cols, X, Y)
        self.ctx.check(self.ctx.lib.alfi_patch_apply_block(self.h, ncol, cp, nx, X.ptr, X.ld, Y.ptr, Y.ld))

    def spmv_block(self, X, Y, cols=None):
        ncol, cp, nx, keep = _block_args(self.n, cols, X, Y)
        self.ctx.check(self.ctx.lib.alfi_spmv_block(self.h, ncol, cp, nx, X.ptr, X.ld, Y.ptr, Y.ld))

    def residual_block(self, B, X, R, cols=None):
        ncol, cp, nx, keep = _block_args(self.n, cols, B, X, R)
        self.ctx.check(self.ctx.lib.alfi_residual_block(self.h, ncol, cp, nx, B.ptr, B.ld, X.ptr, X.ld, R.ptr, R.ld))

    def smooth_block(self, k, B, X, nonzero_guess=True, cols=None):
        ncol, cp, nx, keep = _block_args(self.n, cols, B, X)
        self.ctx.check(self.ctx.lib.alfi_smooth_fgmres_block(self.h, int(k), ncol, cp, nx, B.ptr, B.ld, X.ptr, X.ld,
                                                             1 if nonzero_guess else 0))

    def patch_apply_block_batched(self):
        """Does a block apply of two or more columns on this level, as it stands, take the batched kernel
        (alfi_patch_apply_block_info)?  False: it loops the single apply."""
        b = ctypes.c_int()
        self.ctx.check(self.ctx.lib.alfi_patch_apply_block_info(self.h, ctypes.byref(b)))
        return bool(b.value)

    def patch_apply_block_width(self):
        """The widest batch of a block apply on this level as it stands (alfi_patch_apply_block_width): 4 for dense inverses that
        batch, 4 / 3 / 2 for condensed factors and dense macro stars (what fits ``Context.set_block_lds_bytes``), 0: it loops the
        single apply."""
        w = ctypes.c_int()
        self.ctx.check(self.ctx.lib.alfi_patch_apply_block_width(self.h, ctypes.byref(w)))
        return int(w.value)

    def smooth_block_lockstep(self, k):
        """Does ``smooth_block(k, ...)`` on two or more columns run the smoother's general path in lockstep (one block apply and
        one block product per iteration; alfi_smooth_fgmres_block_info)?  False: the level takes the block form of the four-launch
        iteration or whole smoother calls loop over the columns -- ``smooth_block_mode(k)`` says which."""
        b = ctypes.c_int()
        self.ctx.check(self.ctx.lib.alfi_smooth_fgmres_block_info(self.h, int(k), ctypes.byref(b)))
        return bool(b.value)

    def smooth_block_mode(self, k):
        """Which way ``smooth_block(k, ...)`` goes on two or more columns (alfi_smooth_fgmres_block_mode): 1 the general path in
        lockstep, 2 the block form of the four-launch iteration (the launches per iteration of one column), 0 whole smoother
        calls loop over the columns.  ``smooth_block_lockstep(k)`` is ``smooth_block_mode(k) == 1``."""
        m = ctypes.c_int()
        self.ctx.check(self.ctx.lib.alfi_smooth_fgmres_block_mode(self.h, int(k), ctypes.byref(m)))
        return int(m.value)

    def spmv_block_batched(self):
        """The same for the product and the residual (alfi_spmv_block_info)."""
        b = ctypes.c_int()
        self.ctx.check(self.ctx.lib.alfi_spmv_block_info(self.h, ctypes.byref(b)))
        return bool(b.value)

    def spmv_block_width(self):
        """The widest batch of a block product or residual on this level as it stands (alfi_spmv_block_width): 4 for flat
        operators, 4 / 3 / 2 for de-duplicated ones (what fits ``Context.set_block_lds_bytes``), 0: it loops the single product.
        ``spmv_block_batched`` is True exactly when this is >= 2."""
        w = ctypes.c_int()
        self.ctx.check(self.ctx.lib.alfi_spmv_block_width(self.h, ctypes.byref(w)))
        return int(w.value)

    def set_jacobi(self, on=True):
        """pc_type jacobi (alfi_level_set_jacobi): the level's preconditioner application -- ``patch_apply`` and every smoother --
        becomes y = x / diag(A) (y = x on Dirichlet dofs); such a level needs no patches.  Serial levels only."""
        self.ctx.check(self.ctx.lib.alfi_level_set_jacobi(self.h, 1 if on else 0))

    def smooth_chebyshev(self, k, emin, emax, b, x, nonzero_guess=True):
        """k Chebyshev steps for the interval [emin, emax] on the preconditioned operator (alfi_smooth_chebyshev); x in place."""
        self.ctx.check(self.ctx.lib.alfi_smooth_chebyshev(self.h, int(k), float(emin), float(emax), b.ptr, x.ptr,
                                                          1 if nonzero_guess else 0))

    def arnoldi(self, m, v0):
        """m Arnoldi steps on (preconditioner x operator) from the device vector v0 (alfi_level_arnoldi).  Returns (H, m_done):
        the (m + 1) x m Hessenberg matrix and the number of steps before a breakdown."""
        H = np.zeros((int(m) + 1, int(m)))
        done = ctypes.c_int()
        self.ctx.check(self.ctx.lib.alfi_level_arnoldi(self.h, int(m), v0.ptr, _ptr(H), ctypes.byref(done)))
        return H, done.value

    def set_coarse_inverse(self, inv):
        """inv: dense (n, n) numpy array (copied) or a device pointer (int) that stays owned by the caller."""
        if isinstance(inv, (int, np.integer)):
            self.ctx.check(self.ctx.lib.alfi_coarse_set_inverse(self.h, vp(int(inv)), 1))
        else:
            inv = np.ascontiguousarray(inv, dtype=np.float64)
            assert inv.shape == (self.n, self.n)
            self.ctx.check(self.ctx.lib.alfi_coarse_set_inverse(self.h, _ptr(inv), 0))

    def coarse_factor(self):
        """Dense inverse of this level's operator built by the library itself (blocked Gauss-Jordan on the FP64 matrix cores +
        residual probe, alfi_coarse_factor); returns the probe residual || A X e - e ||."""
        self.ctx.check(self.ctx.lib.alfi_coarse_factor(self.h))
        return self.coarse_residual()

    def coarse_factor_sparse(self, node_coords=None, leaf_nodes=0):
        """Sparse direct factorisation of this level's operator (multifrontal block L D U on a nested-dissection ordering,
        alfi_coarse_factor_sparse) for coarse grids whose dense inverse (8 n^2 bytes) is too large; ``node_coords``
        (nodes, dim) drives the geometric bisection (None: level sets of the graph).  Returns the probe residual."""
        if node_coords is None:
            self.ctx.check(self.ctx.lib.alfi_coarse_factor_sparse(self.h, None, 0, int(leaf_nodes)))
        else:
            xy = np.ascontiguousarray(node_coords, dtype=np.float64)
            assert xy.ndim == 2 and xy.shape[0] * self.bs == self.n, (xy.shape, self.n, self.bs)
            self.ctx.check(self.ctx.lib.alfi_coarse_factor_sparse(self.h, _ptr(xy), int(xy.shape[1]), int(leaf_nodes)))
        return self.coarse_residual()

    def coarse_factor_auto(self, node_coords=None, mode=None, geometric=False):
        """The coarse factorisation the front ends use: ``mode`` "dense", "sparse" or "auto" (sparse from
        ``env.coarse_sparse_min()`` dofs on: dense inverse 8 n^2 bytes and one n x n GEMV per cycle, sparse O(n^{4/3}) bytes
        and ~6 launches per tree height).  The choice is remembered, so a later call without arguments (new operator values,
        every Newton step) repeats it.  The sparse path bisects by graph level sets; ``geometric``: by ``node_coords`` instead
        (measured on ldc3d coarse grids: level sets give 13-15 % less fill, hence the default)."""
        if mode is not None or node_coords is not None or not hasattr(self, "_coarse_choice"):
            self._coarse_choice = (mode or "auto", node_coords if geometric else None)
        mode, node_coords = self._coarse_choice
        if mode == "sparse" or (mode == "auto" and self.n >= env.coarse_sparse_min()):
            rc = self.coarse_factor_sparse(node_coords)
        else:
            rc = self.coarse_factor()
        res = self.coarse_residual()
        if res > 1e-5:         # (the setup fails only beyond ALFI_COARSE_CHECK_FAIL = 1e-2; rounds 1-2 failed at 1e-5)
            import warnings
            warnings.warn("coarse factorisation: probe residual || A X e - e || = %.2e" % res)
        return rc

    def coarse_factor_bytes(self):
        b = ctypes.c_int64()
        self.ctx.check(self.ctx.lib.alfi_coarse_factor_bytes(self.h, ctypes.byref(b)))
        return b.value

    def coarse_residual(self):
        """|| A X e - e ||_inf of the coarse inverse built by ``coarse_factor`` (-1 for a caller-supplied inverse)."""
        w = ctypes.c_double()
        self.ctx.check(self.ctx.lib.alfi_coarse_residual(self.h, ctypes.byref(w)))
        return w.value

    def coarse_solve(self, b, x):
        self.ctx.check(self.ctx.lib.alfi_coarse_solve(self.h, b.ptr, x.ptr))

    def close(self):
        if self.h:
            self.ctx.lib.alfi_level_destroy(self.h)
            self.h = None


class Transfer(object):
    def __init__(self, ctx, coarse, fine, T):
        """T: alfi_amd.problem.TransferData."""
        self.ctx, self.coarse, self.fine = ctx, coarse, fine
        keep = []
        P, PT = _bsr_struct(T.P, keep), _bsr_struct(T.PT, keep)
        PTp = _bsr_struct(T.PT_plain, keep) if T.PT_plain is not T.PT else None
        DI, DIT = _bsr_struct(T.D_I, keep), _bsr_struct(T.D_IT, keep)
        blk = np.ascontiguousarray(T.blk_dofs, dtype=np.int32)
        K = np.ascontiguousarray(T.K_II, dtype=np.float64)
        D = np.ascontiguousarray(T.D_II, dtype=np.float64)
        h = vp()
        ctx.check(ctx.lib.alfi_transfer_create(ctx.h, coarse.h, fine.h, ctypes.byref(P), ctypes.byref(PT),
                                               ctypes.byref(PTp) if PTp is not None else None, ctypes.byref(DI),
                                               ctypes.byref(DIT), blk.shape[0], blk.shape[1], _ptr(blk), _ptr(K),
                                               _ptr(D), ctypes.byref(h)))
        self.h = h
        inj = getattr(T, "inject_map", None)
        serial = not getattr(coarse, "n_own", None) and not getattr(fine, "n_own", None)
        if inj is not None and serial:
            inj = np.ascontiguousarray(inj, dtype=np.int32)
            ctx.check(ctx.lib.alfi_transfer_set_injection(h, _ptr(inj)))
        elif getattr(T, "inject_matrix", None) is not None and serial:
            # non-nested (barycentric) hierarchy: inject = point evaluation at the coarse nodes, a sparse matrix on the device
            import scipy.sparse as sp
            J = sp.csr_matrix(T.inject_matrix)
            J.sort_indices()
            rp = np.ascontiguousarray(J.indptr, dtype=np.int32)
            ci = np.ascontiguousarray(J.indices, dtype=np.int32)
            va = np.ascontiguousarray(J.data, dtype=np.float64)
            st = CsrHost(J.shape[0], J.shape[1], _ptr(rp), _ptr(ci), _ptr(va))
            ctx.check(ctx.lib.alfi_transfer_set_injection_matrix(h, ctypes.byref(st)))

    def inject(self, xf, xc):
        self.ctx.check(self.ctx.lib.alfi_inject(self.h, xf.ptr, xc.ptr))

    def update(self, nu, gamma):
        self.ctx.check(self.ctx.lib.alfi_transfer_update(self.h, float(nu), float(gamma)))

    def block_inverse(self, blk, m):
        out = np.empty((m, m))
        self.ctx.check(self.ctx.lib.alfi_transfer_get_block_inverse(self.h, int(blk), _ptr(out)))
        return out

    def prolong(self, xc, xf):
        self.ctx.check(self.ctx.lib.alfi_prolong(self.h, xc.ptr, xf.ptr))

    def restrict(self, rf, rc, robust=True):
        self.ctx.check(self.ctx.lib.alfi_restrict(self.h, rf.ptr, rc.ptr, 1 if robust else 0))

    def close(self):
        if self.h:
            self.ctx.lib.alfi_transfer_destroy(self.h)
            self.h = None


def coarse_inverse(A_bsr):
    """Dense inverse of the coarsest operator by host LAPACK -- an alternative to ``Level.coarse_factor`` for callers that
    want to supply their own (``Multigrid(..., coarse_inv=...)``); the default path does not use it."""
    A = A_bsr.to_scipy().toarray()
    return np.linalg.inv(A)


def note_patch_level(L, dl):
    """``dl`` holds the patches of the host level ``L`` (a level of the hierarchy, or a rank's dist.LocalLevel): from now on the
    device level records on ``L`` what it stores (``L.patch_storage`` = ``Level.condensed()``, ``L.patch_factor_bytes`` =
    ``Level.factor_bytes()``, ``L.patch_factor_dtype`` = ``Level.patch_storage_dtype()``), whenever that can change -- factor(), set_patch_groups(), set_multiplicative(),
    set_patch_facet_correction().  A level decides at its first factorisation: where the caller factors later (operators formed
    on the device first), the record follows then."""
    dl.host_level = L
    dl._record_storage()


def ask_patch_storage(dl, dtype):
    """The front ends' ``patch_factor_dtype`` keyword on one device level: None asks nothing; "f32" asks the level
    (``Level.set_patch_storage``), and a level the library refuses with ALFI_E_ARG -- it has no FP32 form: the small 2-D stars,
    macro stars, caller-supplied groups -- keeps FP64, which ``L.patch_factor_dtype`` of its host level then records
    (note_patch_level).  Any other error propagates."""
    if dtype is None:
        return
    if dtype != "f32":
        raise ValueError("patch_factor_dtype %r (None or \"f32\")" % (dtype,))
    try:
        dl.set_patch_storage(dtype)
    except AlfiHipError as e:
        if e.code != E_ARG:
            raise


def ask_macro_patch_storage(dl, dtype):
    """The front ends' ``macro_factor_dtype`` keyword on one device level, as ask_patch_storage: None asks nothing; "f32" asks
    the level through ``Level.set_macro_patch_storage``, and a level the library refuses with ALFI_E_ARG (caller-supplied
    groups: the condensed Scott-Vogelius levels; small 2-D stars; multiplicative sweeps) keeps FP64.  Any other error
    propagates."""
    if dtype is None:
        return
    if dtype != "f32":
        raise ValueError("macro_factor_dtype %r (None or \"f32\")" % (dtype,))
    try:
        dl.set_macro_patch_storage(dtype)
    except AlfiHipError as e:
        if e.code != E_ARG:
            raise


def check_factor_dtypes(patch_factor_dtype, macro_factor_dtype):
    """One FP32 request per level: the two keywords of the front ends exclude each other."""
    if patch_factor_dtype is not None and macro_factor_dtype is not None:
        raise ValueError("patch_factor_dtype and macro_factor_dtype are two requests for the same levels: give one")
    if macro_factor_dtype not in (None, "f32"):
        raise ValueError("macro_factor_dtype %r (None or \"f32\")" % (macro_factor_dtype,))


def condense_patches(L):
    """Whether the level's patch factors are stored condensed: the generator supplied group labels (macro-star patches of
    the Scott-Vogelius hierarchy, sv.macro_cell_groups) and ALFI_CONDENSE is not 0 -- or the device level built from ``L``
    found groups by itself when it factored (vertex stars whose dense inverses would be large) and still uses them
    (``L.patch_storage == 2``, recorded by the device level: note_patch_level).  ``L`` may be a rank's local level of a
    partitioned hierarchy (dist.DistMultigrid.local_levels): the decision is the rank's own."""
    if not env.condense():
        return False
    return getattr(L, "patch_groups", None) is not None or getattr(L, "patch_storage", 0) == 2


class Multigrid(object):
    """Device-resident PCMG (solver.py:359-379) built from alfi_amd.problem.build_hierarchy output."""

    def __init__(self, ctx, levels, transfers, k, robust_restriction=False, coarse_inv=None, verbose=False, coarse="auto",
                 patch_factor_dtype=None):
        """coarse: "dense" (explicit inverse, alfi_coarse_factor), "sparse" (multifrontal factors, alfi_coarse_factor_sparse)
        or "auto": sparse from COARSE_SPARSE_MIN dofs on (env ALFI_COARSE_SPARSE_MIN).
        patch_factor_dtype: None, or "f32": every smoothed level is asked to store its dense patch inverses in single precision
        (ask_patch_storage: a level without an FP32 form keeps FP64; ``L.patch_factor_dtype`` records what each one holds)."""
        import time
        t0 = time.time()
        dlevels = []
        for L in levels:
            dl = Level(ctx, L.A, L.bc_dofs)
            if L.level > 0:
                dl.set_patches(L.patch_ptr, L.patch_dofs)
                if getattr(L, "patch_groups", None) is not None and env.condense():
                    dl.set_patch_groups(L.patch_groups)
                elif not env.condense():
                    dl.set_patch_groups(None)              # dense inverses, also where the level would find groups itself
                ask_patch_storage(dl, patch_factor_dtype)
                dl.factor_with_fallback()
                note_patch_level(L, dl)
            elif coarse_inv is not None:
                dl.set_coarse_inverse(coarse_inv)          # an inverse supplied by the caller (numpy array / device pointer)
            else:                                          # the library's own factorisation, dense or multifrontal
                dl.coarse_factor_auto(getattr(getattr(L, "V", None), "node_coords", None), coarse)
            dlevels.append(dl)
        self._from_device_levels(ctx, dlevels, transfers, k, robust_restriction)
        if verbose:
            print("[alfi_amd] device hierarchy ready in %.1fs" % (time.time() - t0), flush=True)

    def _from_device_levels(self, ctx, dlevels, transfers, k, robust_restriction):
        """dlevels: hip.Level objects (level 0 with a coarse inverse, the others with factored patches)."""
        self.ctx = ctx
        self.levels, self.transfers = list(dlevels), []
        for i, T in enumerate(transfers):
            dt = Transfer(ctx, self.levels[i], self.levels[i + 1], T)
            dt.update(T.nu, T.gamma)
            self.transfers.append(dt)
        lv = (vp * len(self.levels))(*[l.h for l in self.levels])
        tr = (vp * max(1, len(self.transfers)))(*[t.h for t in self.transfers])
        h = vp()
        ctx.check(ctx.lib.alfi_mg_create(ctx.h, len(self.levels), lv, tr, int(k), 1 if robust_restriction else 0,
                                         ctypes.byref(h)))
        self.h = h
        self.k = k
        ctx.sync()

    def variant(self, robust_restriction):
        """A second cycle handle (alfi_mg) over the SAME device levels and transfers with the other restriction setting
        (`--restriction`, alfi/driver.py:41); ``close_handle()`` releases it without touching the shared levels."""
        other = Multigrid.__new__(Multigrid)
        other.ctx, other.levels, other.transfers, other.k = self.ctx, self.levels, self.transfers, self.k
        lv = (vp * len(self.levels))(*[l.h for l in self.levels])
        tr = (vp * max(1, len(self.transfers)))(*[t.h for t in self.transfers])
        h = vp()
        self.ctx.check(self.ctx.lib.alfi_mg_create(self.ctx.h, len(self.levels), lv, tr, int(self.k),
                                                   1 if robust_restriction else 0, ctypes.byref(h)))
        other.h = h
        return other

    def close_handle(self):
        if self.h:
            self.ctx.lib.alfi_mg_destroy(self.h)
            self.h = None

    def vcycle(self, b, x):
        self.ctx.check(self.ctx.lib.alfi_mg_vcycle(self.h, b.ptr, x.ptr))

    def fcycle(self, b, x):
        self.ctx.check(self.ctx.lib.alfi_mg_fcycle(self.h, b.ptr, x.ptr))

    def vcycle_block(self, B, X, cols=None):
        """``vcycle`` on the columns of the DeviceMats B and X (alfi_mg_vcycle_block; eager, never a captured graph)."""
        ncol, cp, nx, keep = _block_args(self.levels[-1].n, cols, B, X)
        self.ctx.check(self.ctx.lib.alfi_mg_vcycle_block(self.h, ncol, cp, nx, B.ptr, B.ld, X.ptr, X.ld))

    def fcycle_block(self, B, X, cols=None):
        ncol, cp, nx, keep = _block_args(self.levels[-1].n, cols, B, X)
        self.ctx.check(self.ctx.lib.alfi_mg_fcycle_block(self.h, ncol, cp, nx, B.ptr, B.ld, X.ptr, X.ld))

    SMOOTHERS = {"fgmres": 0, "chebyshev": 1}      # ALFI_SMOOTHER_FGMRES / ALFI_SMOOTHER_CHEBYSHEV
    CYCLES = {"v": 1, "w": 2}

    def set_smoother(self, kind, bounds=None):
        """The level smoother of every cycle (alfi_mg_set_smoother): "fgmres" (default) or "chebyshev" with ``bounds`` = one
        (emin, emax) pair per level 1 .. nlevels-1 (``chebyshev_bounds()``); the number of steps stays ``k``."""
        if kind not in self.SMOOTHERS:
            raise ValueError("smoother %r (fgmres or chebyshev)" % (kind,))
        if kind == "fgmres":
            self.ctx.check(self.ctx.lib.alfi_mg_set_smoother(self.h, 0, None, None))
            return
        b = np.ascontiguousarray(bounds, dtype=np.float64).reshape(-1, 2)
        if b.shape[0] != len(self.levels) - 1:
            raise ValueError("need one (emin, emax) pair per level above the coarsest: %d, got %d" % (len(self.levels) - 1, b.shape[0]))
        emin, emax = np.ascontiguousarray(b[:, 0]), np.ascontiguousarray(b[:, 1])
        self.ctx.check(self.ctx.lib.alfi_mg_set_smoother(self.h, 1, _ptr(emin), _ptr(emax)))

    def set_cycle_type(self, kind):
        """pc_mg_cycle_type (alfi_mg_set_cycles): "v" (default) or "w" -- every level >= 2 recurses twice."""
        if kind not in self.CYCLES:
            raise ValueError("cycle type %r (v or w)" % (kind,))
        self.ctx.check(self.ctx.lib.alfi_mg_set_cycles(self.h, self.CYCLES[kind]))

    def chebyshev_bounds(self, steps=10, esteig=(0.0, 0.1, 0.0, 1.1), seed=0):
        """Chebyshev intervals of the levels 1 .. nlevels-1 the way KSPChebyshevEstEigSet sets them: ``steps`` Arnoldi steps on
        (preconditioner x operator) from the vector ``numpy.random.default_rng(seed).standard_normal(n)`` with the Dirichlet
        entries zeroed; lambda_max / lambda_min = the largest / smallest real part of the Ritz values; the interval is
        (a lambda_min + b lambda_max, c lambda_min + d lambda_max) for esteig = (a, b, c, d).  Returns [(emin, emax), ...].
        The intervals belong to the operators and patch factors of this moment: estimate again after either changes."""
        a, b, c, d = (float(t) for t in esteig)
        out = []
        for L in self.levels[1:]:
            v = np.random.default_rng(seed).standard_normal(L.n)
            dv = self.ctx.vec(v)
            L.zero_bc(dv)
            H, m = L.arnoldi(steps, dv)
            if m < 1:
                raise AlfiHipError("chebyshev_bounds: the Arnoldi iteration broke down at once (zero operator?)")
            ritz = np.linalg.eigvals(H[:m, :m]).real
            lmin, lmax = float(ritz.min()), float(ritz.max())
            out.append((a * lmin + b * lmax, c * lmin + d * lmax))
        return out

    def cg(self, b, x, rtol=1e-8, atol=0.0, max_it=200, full=False):
        """CG with a zero initial guess and the unpreconditioned residual norm on the finest operator, preconditioned by one
        cycle (``full``: the full cycle) per iteration (alfi_mg_cg).  Returns (iterations, recurrence residual norm)."""
        its, rn = ctypes.c_int(), ctypes.c_double()
        self.ctx.check(self.ctx.lib.alfi_mg_cg(self.h, b.ptr, x.ptr, float(rtol), float(atol), int(max_it), 1 if full else 0,
                                               ctypes.byref(its), ctypes.byref(rn)))
        return its.value, rn.value

    def close(self):
        if self.h:
            self.ctx.lib.alfi_mg_destroy(self.h)
            self.h = None
        for t in self.transfers:
            t.close()
        for l in self.levels:
            l.close()


class RawVec(object):
    """A device buffer owned by someone else (a torch tensor, a slice of a DeviceVec) in the shape the wrappers expect
    (``.ptr``); with a ctx it can be filled and read like a DeviceVec."""

    def __init__(self, ptr, n, ctx=None, parent=None):
        self.ptr, self.n, self.ctx, self._parent = vp(int(ptr)), int(n), ctx, parent

    def set(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        assert a.shape == (self.n,)
        self.ctx.check(self.ctx.lib.alfi_memcpy_h2d(self.ctx.h, self.ptr, _ptr(a), self.n * 8))

    def get(self):
        out = np.empty(self.n, dtype=np.float64)
        self.ctx.check(self.ctx.lib.alfi_memcpy_d2h(self.ctx.h, _ptr(out), self.ptr, self.n * 8))
        return out


def view(v, off, n):
    """Entries [off, off + n) of a device vector as a vector of its own (no copy; keeps its parent alive)."""
    assert 0 <= off and off + n <= v.n
    return RawVec(v.ptr.value + 8 * int(off), n, ctx=getattr(v, "ctx", None), parent=v)


class Csr(object):
    """Scalar CSR matrix on the device (alfi_csr_*): the rank's rows of the discrete divergence and its transpose."""

    def __init__(self, ctx, M):
        import scipy.sparse as sp
        M = sp.csr_matrix(M)
        M.sort_indices()
        rp = np.ascontiguousarray(M.indptr, dtype=np.int32)
        ci = np.ascontiguousarray(M.indices, dtype=np.int32)
        va = np.ascontiguousarray(M.data, dtype=np.float64)
        st = CsrHost(M.shape[0], M.shape[1], _ptr(rp), _ptr(ci), _ptr(va))
        self.ctx, self.shape = ctx, M.shape
        h = vp()
        ctx.check(ctx.lib.alfi_csr_create(ctx.h, ctypes.byref(st), ctypes.byref(h)))
        self.h = h

    def mult(self, x, y, b=None, alpha=1.0, mode=0):
        """mode 0: y = M x;  1: y = b - alpha M x;  2: y += M x;  3: y = alpha M x"""
        self.ctx.check(self.ctx.lib.alfi_csr_mult(self.h, x.ptr, y.ptr, b.ptr if b is not None else None, float(alpha),
                                                  int(mode)))

    def close(self):
        if self.h:
            self.ctx.lib.alfi_csr_destroy(self.h)
            self.h = None


class Saddle(object):
    """Outer solve of one Newton step (alfi/solver.py:386-422): FGMRES around PCFIELDSPLIT-Schur-full with the device
    multigrid as fieldsplit_0 and DGMassInv (solver.py:15-38) as fieldsplit_1."""

    def __init__(self, mg, B, mass_diag, nu, gamma, remove_constant_nullspace=True, mass_inv=None, n_u=None):
        """mg: hip.Multigrid; B: scipy CSR (pressure dofs x velocity dofs); mass_diag: diagonal of the P0 mass matrix;
        mass_inv: scipy sparse inverse of a block-diagonal (discontinuous P_k) pressure mass matrix, replaces mass_diag.
        On a PARTITIONED finest level (alfi_amd.dist) B holds the rank's pressure rows over all local velocity dofs (owned
        + ghost), n_u = the owned velocity dofs (vectors are (owned velocity | owned pressure)) and the call is collective."""
        import scipy.sparse as sp
        self.mg, self.ctx = mg, mg.ctx
        B = sp.csr_matrix(B)
        B.sort_indices()
        BT = B.T.tocsr()
        BT.sort_indices()
        keep = []

        def st(M):
            rp = np.ascontiguousarray(M.indptr, dtype=np.int32)
            ci = np.ascontiguousarray(M.indices, dtype=np.int32)
            va = np.ascontiguousarray(M.data, dtype=np.float64)
            keep.extend([rp, ci, va])
            return CsrHost(M.shape[0], M.shape[1], _ptr(rp), _ptr(ci), _ptr(va))
        sB, sBT = st(B), st(BT)
        if mass_diag is None:
            mass_diag = np.ones(B.shape[0])
        md = np.ascontiguousarray(mass_diag, dtype=np.float64)
        h = vp()
        self.ctx.check(self.ctx.lib.alfi_saddle_create(mg.h, ctypes.byref(sB), ctypes.byref(sBT), _ptr(md), float(nu),
                                                       float(gamma), 1 if remove_constant_nullspace else 0,
                                                       ctypes.byref(h)))
        self.h = h
        self.n_u, self.n_p = (B.shape[1] if n_u is None else int(n_u)), B.shape[0]
        self.n = self.n_u + self.n_p
        if mass_inv is not None:
            Mi = sp.csr_matrix(mass_inv)
            Mi.sort_indices()
            sM = st(Mi)
            self.ctx.check(self.ctx.lib.alfi_saddle_set_mass_inverse(self.h, ctypes.byref(sM)))

    def update(self, nu, gamma):
        self.ctx.check(self.ctx.lib.alfi_saddle_update(self.h, float(nu), float(gamma)))

    def dot(self, x, y):
        """x . y of two (velocity | pressure) device vectors, summed over the ranks on partitioned levels (alfi_saddle_dot)."""
        out = ctypes.c_double()
        self.ctx.check(self.ctx.lib.alfi_saddle_dot(self.h, x.ptr, y.ptr, ctypes.byref(out)))
        return out.value

    def mult(self, x, y):
        self.ctx.check(self.ctx.lib.alfi_saddle_mult(self.h, x.ptr, y.ptr))

    def precond(self, x, y):
        self.ctx.check(self.ctx.lib.alfi_saddle_precond(self.h, x.ptr, y.ptr))

    VELOCITY_SOLVERS = {"mg": 0, "direct": 1}      # ALFI_VELOCITY_MG / ALFI_VELOCITY_DIRECT

    def set_velocity_solver(self, kind):
        """fieldsplit_0: "mg" (one full cycle of ``mg``, the default) or "direct" (exact solve with multifrontal factors of the
        finest operator -- solver_type allu; ``factor_velocity`` after every change of that operator).  Switching back to "mg"
        releases the factors.  A partitioned finest level refuses "direct" (AlfiHipError, ALFI_E_STATE)."""
        if kind not in self.VELOCITY_SOLVERS:
            raise ValueError("velocity solver %r (mg or direct)" % (kind,))
        self.ctx.check(self.ctx.lib.alfi_saddle_set_velocity_solver(self.h, self.VELOCITY_SOLVERS[kind]))
        self.velocity_solver = kind

    def factor_velocity(self, node_coords=None, leaf_nodes=0, max_bytes=0):
        """Factor the finest operator's current values for the direct fieldsplit_0 (symbolic plan kept from the first call);
        ``max_bytes`` > 0 caps factors + front storage (the free device memory caps them always).  Returns the residual probe
        || A x - e ||_inf of the new factors."""
        if node_coords is None:
            self.ctx.check(self.ctx.lib.alfi_saddle_factor_velocity(self.h, None, 0, int(leaf_nodes), int(max_bytes)))
        else:
            xy = np.ascontiguousarray(node_coords, dtype=np.float64)
            self.ctx.check(self.ctx.lib.alfi_saddle_factor_velocity(self.h, _ptr(xy), int(xy.shape[1]), int(leaf_nodes),
                                                                    int(max_bytes)))
        return self.velocity_info()[1]

    def velocity_info(self):
        """(device bytes of the direct velocity factors, probe residual of the last factorisation)."""
        b, r = ctypes.c_int64(), ctypes.c_double()
        self.ctx.check(self.ctx.lib.alfi_saddle_velocity_info(self.h, ctypes.byref(b), ctypes.byref(r)))
        return b.value, r.value

    def velocity_solve(self, b, x):
        """x = A^-1 b with the direct velocity factors (device vectors of the finest level's length)."""
        self.ctx.check(self.ctx.lib.alfi_saddle_velocity_solve(self.h, b.ptr, x.ptr))

    def solve(self, b, x, rtol=1e-8, atol=1e-8, max_it=500, restart=30):
        """Returns (iterations, true residual norm)."""
        its, rn = ctypes.c_int(), ctypes.c_double()
        self.ctx.check(self.ctx.lib.alfi_saddle_solve(self.h, b.ptr, x.ptr, float(rtol), float(atol), int(max_it),
                                                      int(restart), ctypes.byref(its), ctypes.byref(rn)))
        return its.value, rn.value

    # block right-hand sides (DeviceMats of n_u + n_p rows; cols: the columns to work on, None = all) -- column c of every
    # result is the single call on column c bit for bit
    def mult_block(self, X, Y, cols=None):
        ncol, cp, nx, keep = _block_args(self.n, cols, X, Y)
        self.ctx.check(self.ctx.lib.alfi_saddle_mult_block(self.h, ncol, cp, nx, X.ptr, X.ld, Y.ptr, Y.ld))

    def precond_block(self, X, Y, cols=None):
        ncol, cp, nx, keep = _block_args(self.n, cols, X, Y)
        self.ctx.check(self.ctx.lib.alfi_saddle_precond_block(self.h, ncol, cp, nx, X.ptr, X.ld, Y.ptr, Y.ld))

    def solve_block(self, B, X, rtol=1e-8, atol=1e-8, max_it=500, restart=30, cols=None):
        """``solve`` on the listed columns in lockstep (alfi_saddle_solve_block): every column has its own tolerance
        max(rtol |b_c|, atol), iteration count and restarts, and drops out when it has converged.  Returns (iterations,
        true residual norms), one entry per listed column."""
        ncol, cp, nx, keep = _block_args(self.n, cols, B, X)
        its, rn = np.zeros(max(ncol, 1), dtype=np.int32), np.zeros(max(ncol, 1))
        self.ctx.check(self.ctx.lib.alfi_saddle_solve_block(self.h, ncol, cp, nx, B.ptr, B.ld, X.ptr, X.ld, float(rtol), float(atol),
                                                            int(max_it), int(restart), _ptr(its), _ptr(rn)))
        return [int(i) for i in its[:ncol]], [float(r) for r in rn[:ncol]]

    def close(self):
        if self.h:
            self.ctx.lib.alfi_saddle_destroy(self.h)
            self.h = None


def supg_load(V, f, nq=None):
    """The body force ``f(points (N, dim)) -> (N, dim)`` at the physical points of the SUPG / GLS rule on V's cells: the
    (ncell, nq, dim) table of ``Level.set_supg_load`` and of ``_hostlib.supg(..., fq=)``."""
    from . import _hostlib
    x = _hostlib.supg_points(V, nq)
    nc, nq_, d = x.shape
    return np.ascontiguousarray(np.asarray(f(x.reshape(-1, d)), dtype=np.float64).reshape(nc, nq_, d))
