"""ctypes binding of libalfi_host.so (CPU operator generator, csrc/host_assemble.cpp).  Input generation only."""
import ctypes
import os
import numpy as np

from . import env

_lib = None


def cpu_share():
    """CPUs this process may actually use: the affinity mask capped by the cgroup CPU quota (a GPU box hands out a share
    of its cores; OpenMP teams larger than the quota are throttled into the ground)."""
    n = len(os.sched_getaffinity(0))
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            txt = open(path).read().split()
            if path.endswith("cpu.max"):
                if txt[0] != "max":
                    n = min(n, max(1, int(float(txt[0]) / float(txt[1]) + 0.5)))
            else:
                q = float(txt[0])
                per = float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
                if q > 0:
                    n = min(n, max(1, int(q / per + 0.5)))
            break
        except (OSError, ValueError, IndexError):
            continue
    return n


def lib():
    global _lib
    if _lib is None:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libalfi_host.so")
        if not os.path.exists(path):
            from . import build
            build.build_host()
        _lib = ctypes.CDLL(path)
        _lib.alfi_host_node_graph.restype = ctypes.c_int
        _lib.alfi_host_assemble_bsr.restype = ctypes.c_int
        _lib.alfi_host_apply_bc_bsr.restype = ctypes.c_int
        _lib.alfi_host_extract_blocks.restype = ctypes.c_int
        _lib.alfi_host_interior_blocks.restype = ctypes.c_int
        _lib.alfi_host_bsr_transpose.restype = ctypes.c_int
        _lib.alfi_host_supg.restype = ctypes.c_int
        _lib.alfi_host_gls.restype = ctypes.c_int
        _lib.alfi_host_burman.restype = ctypes.c_int
        _lib.alfi_host_find_groups.restype = ctypes.c_int64
        _lib.alfi_host_f32_index_table.restype = None
        _lib.alfi_host_piece_index_table.restype = None
        _lib.alfi_host_patch_index_table.restype = None
        for name in ("patch_layout", "condensed", "sweep", "sweep_condensed", "f32_layout", "macro_f32_layout", "f32_ranges"):
            getattr(_lib, "alfi_host_plan_" + name).restype = ctypes.c_void_p
        _lib.alfi_host_f32_index.restype = ctypes.c_int64
        _lib.alfi_host_f32_ld.restype = ctypes.c_int
        _lib.alfi_host_f32_patch_floats.restype = ctypes.c_int64
        _lib.alfi_host_plan_status.restype = ctypes.c_int
        _lib.alfi_host_plan_table.restype = ctypes.c_int
        _lib.alfi_host_plan_free.restype = None
        nthr = env.host_threads() or cpu_share()
        _lib.alfi_host_set_num_threads(ctypes.c_int(nthr))
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def find_groups(bs, rowptr, colidx, patch_ptr, patch_dofs):
    """Group labels for condensed patch factors from the block sparsity alone (csrc/find_groups.h, the rule of
    alfi_patches_find_groups): one label per entry of ``patch_dofs``, -1 = skeleton."""
    rp = np.ascontiguousarray(rowptr, dtype=np.int32)
    ci = np.ascontiguousarray(colidx, dtype=np.int32)
    pp = np.ascontiguousarray(patch_ptr, dtype=np.int64)
    pd = np.ascontiguousarray(patch_dofs, dtype=np.int32)
    out = np.empty(len(pd), dtype=np.int32)
    lib().alfi_host_find_groups(ctypes.c_int(bs), ctypes.c_int64(len(rp) - 1), ctypes.c_int64(len(pp) - 1), _p(pp), _p(pd),
                                _p(rp), _p(ci), _p(out))
    return out


class PlanError(ValueError):
    """A planner of csrc/patch_plan.h refused its input: ``code`` is the ALFI_E_* code the device library returns for it, the
    message its error text."""

    def __init__(self, code, message):
        ValueError.__init__(self, message)
        self.code = code


# CondChunk (csrc/cond_layout.h)
COND_CHUNK = np.dtype([(k, np.int64) for k in ("off", "ubase", "sidx0", "stage_off")]
                      + [(k, np.int32) for k in ("xq0", "xq1", "bq0", "bq1", "e0", "ne", "u0", "nu", "nI", "xp0", "bp0", "pad")])
_PLAN_DTYPES = {4: np.dtype(np.int32), 8: np.dtype(np.int64), COND_CHUNK.itemsize: COND_CHUNK}


def _plan_dict(handle):
    """Every table (a copy, as an array) and scalar (an int) of a plan handle by its name; the handle is released."""
    L = lib()
    h = ctypes.c_void_p(handle)
    try:
        msg = ctypes.c_char_p()
        rc = L.alfi_host_plan_status(h, ctypes.byref(msg))
        if rc != 0:
            raise PlanError(rc, msg.value.decode())
        out, i = {}, 0
        name, ptr, count, item = ctypes.c_char_p(), ctypes.c_void_p(), ctypes.c_int64(), ctypes.c_int()
        while L.alfi_host_plan_table(h, ctypes.c_int64(i), ctypes.byref(name), ctypes.byref(ptr), ctypes.byref(count),
                                     ctypes.byref(item)) == 0:
            dt = _PLAN_DTYPES[item.value]
            n = 1 if count.value < 0 else count.value
            a = np.frombuffer(ctypes.string_at(ptr.value, n * dt.itemsize) if n else b"", dtype=dt).copy()
            out[name.value.decode()] = int(a[0]) if count.value < 0 else a
            i += 1
        return out
    finally:
        L.alfi_host_plan_free(h)


def _patch_args(patch_ptr, patch_dofs):
    pp = np.ascontiguousarray(patch_ptr, dtype=np.int64)
    pd = np.ascontiguousarray(patch_dofs, dtype=np.int32)
    return pp, pd, ctypes.c_int64(len(pp) - 1)


def plan_patch_layout(n, patch_ptr, patch_dofs):
    """The tables alfi_patches_set builds for a level of n dofs (csrc/patch_plan.h: plan_patch_layout) as a dict."""
    pp, pd, npatch = _patch_args(patch_ptr, patch_dofs)
    return _plan_dict(lib().alfi_host_plan_patch_layout(ctypes.c_int64(n), npatch, _p(pp), _p(pd)))


def plan_f32_layout(patch_ptr):
    """The single-precision storage of a level's dense inverses (csrc/patch_plan.h: plan_f32_offsets) as a dict: ``f32_ptr``
    (offsets of the patches in floats), ``inv32_floats``, ``rows_per_load`` (rows of a column one lane loads) and
    ``align_floats`` (every offset is a multiple)."""
    pp = np.ascontiguousarray(patch_ptr, dtype=np.int64)
    return _plan_dict(lib().alfi_host_plan_f32_layout(ctypes.c_int64(len(pp) - 1), _p(pp)))


def plan_macro_f32_layout(patch_ptr):
    """plan_f32_layout for the levels of alfi_patches_set_macro_storage: patches of up to 4096 dofs, same layout."""
    pp = np.ascontiguousarray(patch_ptr, dtype=np.int64)
    return _plan_dict(lib().alfi_host_plan_macro_f32_layout(ctypes.c_int64(len(pp) - 1), _p(pp)))


def plan_f32_ranges(inv_ptr, cap_doubles):
    """The patch ranges an FP32 level of big patches is factored in through a work buffer of ``cap_doubles`` doubles
    (csrc/patch_plan.h: plan_f32_ranges) as a dict: ``ranges`` (the boundaries, 0 .. npatch) and ``work_doubles`` (the largest
    range).  ``inv_ptr``: the offsets of the FP64 inverses, as ``plan_patch_layout`` returns them."""
    ip = np.ascontiguousarray(inv_ptr, dtype=np.int64)
    return _plan_dict(lib().alfi_host_plan_f32_ranges(ctypes.c_int64(len(ip) - 1), _p(ip), ctypes.c_int64(cap_doubles)))


def f32_index_table(n):
    """f32_index(n) computed in one call (macro stars: up to 4096 x 4096 offsets)."""
    L = lib()
    ld = L.alfi_host_f32_ld(ctypes.c_int(n))
    idx = np.empty((ld, n), dtype=np.int64)
    L.alfi_host_f32_index_table(ctypes.c_int(n), _p(idx))
    return ld, L.alfi_host_f32_patch_floats(ctypes.c_int(n)), idx


def piece_index_table(n, ld, min_rows):
    """(ld, n) offsets of the row-piece storage of an n x n inverse with rows padded to ld (csrc/patch_plan.h: piece_index)."""
    idx = np.empty((ld, n), dtype=np.int64)
    lib().alfi_host_piece_index_table(ctypes.c_int(n), ctypes.c_int(ld), ctypes.c_int(min_rows), _p(idx))
    return idx


def patch_index_table(n):
    """The same through the FP64 wrapper (patch_inv_index): rows padded to even."""
    ld = (n + 1) // 2 * 2
    idx = np.empty((ld, n), dtype=np.int64)
    lib().alfi_host_patch_index_table(ctypes.c_int(n), ctypes.c_int(ld), _p(idx))
    return idx


def f32_index(n):
    """(ld, floats, index): the padded row count of an n x n inverse in the single-precision storage, the floats the patch
    occupies and the (ld, n) array of the offsets of its entries (r, c), pad rows r >= n included (f32_inv_index)."""
    L = lib()
    ld = L.alfi_host_f32_ld(ctypes.c_int(n))
    idx = np.array([[L.alfi_host_f32_index(ctypes.c_int(r), ctypes.c_int(c), ctypes.c_int(n)) for c in range(n)]
                    for r in range(ld)], dtype=np.int64).reshape(ld, n)
    return ld, L.alfi_host_f32_patch_floats(ctypes.c_int(n)), idx


def plan_condensed(bs, rowptr, colidx, patch_ptr, patch_dofs, groups):
    """The tables alfi_patches_set_groups builds from the labels ``groups`` (csrc/patch_plan.h: plan_condensed) as a dict."""
    rp = np.ascontiguousarray(rowptr, dtype=np.int32)
    ci = np.ascontiguousarray(colidx, dtype=np.int32)
    pp, pd, npatch = _patch_args(patch_ptr, patch_dofs)
    g = np.ascontiguousarray(groups, dtype=np.int32)
    assert len(g) == len(pd)
    return _plan_dict(lib().alfi_host_plan_condensed(ctypes.c_int(bs), ctypes.c_int64(len(rp) - 1), npatch, _p(pp), _p(pd), _p(g),
                                                     _p(rp), _p(ci)))


def plan_sweep(bs, rowptr, colidx, patch_ptr, patch_dofs, iterset, symmetrise):
    """The schedule alfi_patches_set_multiplicative builds (csrc/patch_plan.h: check_sweep + plan_sweep) as a dict."""
    rp = np.ascontiguousarray(rowptr, dtype=np.int32)
    ci = np.ascontiguousarray(colidx, dtype=np.int32)
    pp, pd, npatch = _patch_args(patch_ptr, patch_dofs)
    it = np.ascontiguousarray(iterset, dtype=np.int64)
    return _plan_dict(lib().alfi_host_plan_sweep(ctypes.c_int(bs), ctypes.c_int64(len(rp) - 1), npatch, _p(pp), _p(pd), _p(rp),
                                                 _p(ci), ctypes.c_int64(len(it)), _p(it), ctypes.c_int(1 if symmetrise else 0)))


def plan_sweep_condensed(bs, patch_ptr, patch_dofs, sweep, cond):
    """The work lists alfi_patches_set_multiplicative_condensed builds per dependency wavefront (csrc/patch_plan.h:
    plan_sweep_condensed) from the dicts ``sweep`` of ``plan_sweep`` and ``cond`` of ``plan_condensed``, as a dict: ``gchunk`` /
    ``wk_ptr`` (group chunks), ``schunk`` / ``wc_ptr`` (sigma chunks), ``node`` / ``wn_ptr`` (block rows of the residual)."""
    pp, pd, npatch = _patch_args(patch_ptr, patch_dofs)
    wp = np.ascontiguousarray(sweep["wave_ptr"], dtype=np.int64)
    seq = np.ascontiguousarray(sweep["seq"], dtype=np.int32)
    gcptr = np.ascontiguousarray(cond["gcptr"], dtype=np.int64)
    chptr = np.ascontiguousarray(cond["chptr"], dtype=np.int64)
    assert len(gcptr) == len(pp) and len(chptr) == len(pp) and wp[-1] == len(seq)
    return _plan_dict(lib().alfi_host_plan_sweep_condensed(ctypes.c_int(bs), npatch, _p(pp), _p(pd), ctypes.c_int64(len(wp) - 1),
                                                           _p(wp), _p(seq), _p(gcptr), _p(chptr)))


def node_graph(cell_nodes, nnode):
    cn = np.ascontiguousarray(cell_nodes, dtype=np.int32)
    ncell, nloc = cn.shape
    rowptr = np.zeros(nnode + 1, dtype=np.int32)
    rc = lib().alfi_host_node_graph(ctypes.c_int64(ncell), ctypes.c_int(nloc), _p(cn), ctypes.c_int64(nnode),
                                    _p(rowptr), None)
    if rc != 0:
        raise RuntimeError("node graph exceeds int32 indexing")
    colidx = np.empty(rowptr[-1], dtype=np.int32)
    lib().alfi_host_node_graph(ctypes.c_int64(ncell), ctypes.c_int(nloc), _p(cn), ctypes.c_int64(nnode), _p(rowptr),
                               _p(colidx))
    return rowptr, colidx


def assemble_bsr(cell_nodes, g, vol, tensors, d, rowptr, colidx, nu=0.0, gamma=0.0, adv=0.0, wind=None, out=None,
                 row_map=None, gamma_full=0.0):
    """gamma: coefficient of (cell_avg div u, div v) (PkP0 forms); gamma_full: of (div u, div v) (Scott-Vogelius forms)."""
    cn = np.ascontiguousarray(cell_nodes, dtype=np.int32)
    ncell, nloc = cn.shape
    g = np.ascontiguousarray(g, dtype=np.float64)
    vol = np.ascontiguousarray(vol, dtype=np.float64)
    S, bI, T1 = (np.ascontiguousarray(tensors[k], dtype=np.float64) for k in ("S", "bI", "T1"))
    if wind is not None:
        wind = np.ascontiguousarray(wind, dtype=np.float64)
    if out is None:
        out = np.zeros((colidx.shape[0], d, d), dtype=np.float64)
    if row_map is not None:
        row_map = np.ascontiguousarray(row_map, dtype=np.int32)
    rc = lib().alfi_host_assemble_bsr(ctypes.c_int64(ncell), ctypes.c_int(nloc), ctypes.c_int(d), _p(cn), _p(g),
                                      _p(vol), _p(S), _p(bI), _p(T1), _p(wind), ctypes.c_double(nu),
                                      ctypes.c_double(gamma), ctypes.c_double(adv), _p(row_map), _p(rowptr), _p(colidx),
                                      _p(out), ctypes.c_double(gamma_full))
    if rc != 0:
        raise RuntimeError("assemble_bsr failed (%d): sparsity pattern does not cover the mesh" % rc)
    return out


def cell_size(mesh):
    """Firedrake's ``CellSize`` = 2 * circumradius [3P] (problem.mesh_size(u, "cell"), alfi/problem.py:46-52)."""
    x = mesh.coords[mesh.cells]
    if mesh.dim == 2:
        a = np.linalg.norm(x[:, 1] - x[:, 2], axis=1)
        b = np.linalg.norm(x[:, 0] - x[:, 2], axis=1)
        c = np.linalg.norm(x[:, 0] - x[:, 1], axis=1)
        area = mesh.cell_geometry()[1]
        return 2.0 * a * b * c / (4.0 * area)
    e = lambda i, j: np.linalg.norm(x[:, i] - x[:, j], axis=1)
    aA, bB, cC = e(0, 1) * e(2, 3), e(0, 2) * e(1, 3), e(0, 3) * e(1, 2)         # products of opposite edges
    vol = mesh.cell_geometry()[1]
    rad = np.sqrt((aA + bB + cC) * (aA + bB - cC) * (aA - bB + cC) * (-aA + bB + cC)) / (24.0 * vol)
    return 2.0 * rad


def supg_rule(V, nq=None):
    """(lam, wq): the quadrature rule of the SUPG / GLS terms on the space V -- degree 2k, n points per direction, exact to
    2n - 1 >= 2k (the rule of ``supg``, ``gls`` and hip.DeviceLevel.set_supg)."""
    from .elements import simplex_quadrature
    el = V.element
    deg = 3 if (el.bubble or el.degree == 3) else el.degree                  # ufl degree of the (enriched) element
    return simplex_quadrature(V.dim, nq or (deg + 1))


def supg_points(V, nq=None):
    """Physical coordinates (ncell, nq, dim) of the points of ``supg_rule`` in every cell of V's mesh, in rule order."""
    lam, _ = supg_rule(V, nq)
    m = V.mesh
    return np.einsum("qv,cvx->cqx", lam, m.coords[m.cells])


def _stabilisation(V, U, W, nu, weight, magic, rowptr, colidx, vals, F, nq, fq):
    mesh, el, d = V.mesh, V.element, V.dim
    lam, wq = supg_rule(V, nq)
    phi, dphi = el.tabulate(lam)
    d2phi = el.tabulate_hessian(lam)
    g, vol = mesh.cell_geometry()
    h = cell_size(mesh)
    cn = np.ascontiguousarray(V.cell_nodes, dtype=np.int32)
    U = np.ascontiguousarray(U, dtype=np.float64)
    if fq is not None:
        fq = np.ascontiguousarray(fq, dtype=np.float64)
        assert fq.shape == (cn.shape[0], len(wq), d), "body force table must be (ncell, nq, dim) in supg_rule order"
    arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (g, vol, h, wq, phi, dphi, d2phi)]
    head = (ctypes.c_int64(cn.shape[0]), ctypes.c_int(cn.shape[1]), ctypes.c_int(d), _p(cn), _p(arrs[0]), _p(arrs[1]),
            _p(arrs[2]), ctypes.c_int(len(wq)), _p(arrs[3]), _p(arrs[4]), _p(arrs[5]), _p(arrs[6]), _p(U))
    tail = (ctypes.c_double(nu), ctypes.c_double(weight), ctypes.c_double(magic), _p(rowptr), _p(colidx), _p(vals), _p(F),
            _p(fq))
    if W is None:
        rc = lib().alfi_host_supg(*head, *tail)
    else:
        W = np.ascontiguousarray(W, dtype=np.float64)
        assert W.size == U.size, "the wind has the state's shape"
        rc = lib().alfi_host_gls(*head, _p(W), *tail)
    if rc != 0:
        raise RuntimeError("%s failed (%d): sparsity pattern does not cover the mesh" % ("supg" if W is None else "gls", rc))


def supg(V, U, nu, weight, magic, rowptr=None, colidx=None, vals=None, F=None, nq=None, fq=None):
    """SUPG stabilisation (stabilisation.py:47-97, solver.py:204-234) about the state U (num_nodes, dim): adds the residual
    contribution to F (num_dofs) and / or the Newton linearisation to the BSR values ``vals``.  Quadrature degree 2k.
    fq (ncell, nq, dim): the body force at the points of ``supg_rule`` (subtracted in the strong residual, solver.py:216-217)."""
    _stabilisation(V, U, None, nu, weight, magic, rowptr, colidx, vals, F, nq, fq)


def gls(V, U, W, nu, weight, magic, rowptr=None, colidx=None, vals=None, F=None, nq=None, fq=None):
    """GLS stabilisation (stabilisation.py:47-97, solver.py:204-234): weight beta (Lu - f, L_W v) with the strong operator
    applied to the test function about the wind W (num_nodes, dim; the state at the start of the solve, not differentiated).
    Same contract as ``supg``."""
    _stabilisation(V, U, W, nu, weight, magic, rowptr, colidx, vals, F, nq, fq)


def burman(table, U, weight, lists, vals=None, F=None, beta=None):
    """Burman interior-penalty stabilisation (stabilisation.py:139-162, alfi_amd/burman.py) about the state U (nstate,
    dim): adds the residual contribution to F (rows x dim) and / or the Newton linearisation to the BSR values ``vals``.
    ``table``: burman.FacetTable of the level; ``lists``: its contributor lists for the level's sparsity
    (FacetTable.contributors); ``beta`` (nfacet, may be None): receives beta_F of every facet.  The state may be longer than
    the rows (a rank-local table of a partitioned level: local nodes first, then the other nodes its facets reach)."""
    (bptr, bfac, bab), (nptr, nfac, na) = lists
    t = table
    U = np.ascontiguousarray(U, dtype=np.float64)
    nrow = len(nptr) - 1
    assert U.size % t.d == 0 and U.size >= nrow * t.d
    assert t.nf == 0 or (int(t.union.min()) >= 0 and int(t.union.max()) < U.size // t.d), "facet node beyond the state"
    if vals is not None:
        assert vals.shape == (len(bptr) - 1, t.d, t.d) and vals.flags.c_contiguous and vals.dtype == np.float64
    if F is not None:
        assert F.shape == (nrow * t.d,) and F.flags.c_contiguous and F.dtype == np.float64
    if beta is not None:
        assert beta.shape == (t.nf,) and beta.flags.c_contiguous and beta.dtype == np.float64
    arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (t.J, t.area, t.coef, t.ws, t.wn, t.phin)]
    rc = lib().alfi_host_burman(ctypes.c_int64(t.nf), ctypes.c_int(t.nu), ctypes.c_int(t.nloc), ctypes.c_int(t.d),
                                ctypes.c_int(len(t.ws)), ctypes.c_int(len(t.wn)), _p(t.union), _p(t.cfg), _p(arrs[0]),
                                _p(arrs[1]), _p(arrs[2]), _p(arrs[3]), _p(arrs[4]), _p(arrs[5]), _p(U),
                                ctypes.c_double(weight), ctypes.c_int64(len(bptr) - 1), _p(bptr), _p(bfac), _p(bab),
                                _p(vals), ctypes.c_int64(len(nptr) - 1), _p(nptr), _p(nfac), _p(na), _p(F), _p(beta))
    if rc != 0:
        raise RuntimeError("burman failed (%d)" % rc)


def contributors(cell_nodes, nnode, rowptr, colidx, nindex=None, partial=False):
    """(cptr int64 (nnzb + 1), ccell int32, cba uint16): for every BSR block the (cell, b * nloc + a) pairs that contribute to
    it, in a fixed order -- the gather lists of the device assembly (alfi_level_set_assembly).  nindex: cell_nodes may index
    up to nindex > nnode nodes (only the first nnode have operator rows); partial: pairs without a block are skipped (a
    rank's ghost rows hold local columns only)."""
    cn = np.ascontiguousarray(cell_nodes, dtype=np.int32)
    ncell, nloc = cn.shape
    if nloc * nloc > 65535:
        raise ValueError("element with %d nodes: the pair code does not fit 16 bits" % nloc)
    rowptr = np.ascontiguousarray(rowptr, dtype=np.int32)
    colidx = np.ascontiguousarray(colidx, dtype=np.int32)
    cptr = np.zeros(colidx.shape[0] + 1, dtype=np.int64)
    fn = lib().alfi_host_contributors
    fn.restype = ctypes.c_int
    tail = (ctypes.c_int64(int(nindex) if nindex is not None else int(nnode)), ctypes.c_int(1 if partial else 0))
    rc = fn(ctypes.c_int64(ncell), ctypes.c_int(nloc), _p(cn), ctypes.c_int64(nnode), _p(rowptr), _p(colidx), _p(cptr), None, None,
            *tail)
    if rc != 0:
        raise RuntimeError("contributors failed (%d): sparsity pattern does not cover the mesh" % rc)
    assert partial or cptr[-1] == ncell * nloc * nloc
    ccell = np.empty(cptr[-1], dtype=np.int32)
    cba = np.empty(cptr[-1], dtype=np.uint16)
    fn(ctypes.c_int64(ncell), ctypes.c_int(nloc), _p(cn), ctypes.c_int64(nnode), _p(rowptr), _p(colidx), _p(cptr), _p(ccell), _p(cba),
       *tail)
    return cptr, ccell, cba


def apply_bc_bsr(nrow, d, rowptr, colidx, vals, bcmask, row_ids=None):
    """Dirichlet rows / columns -> identity.  row_ids: the node of each block row when the rows are a subset."""
    bcmask = np.ascontiguousarray(bcmask, dtype=np.uint8)
    if row_ids is not None:
        row_ids = np.ascontiguousarray(row_ids, dtype=np.int32)
    lib().alfi_host_apply_bc_bsr(ctypes.c_int64(nrow), ctypes.c_int(d), _p(rowptr), _p(colidx), _p(vals), _p(bcmask),
                                 _p(row_ids))


def extract_blocks(d, rowptr, colidx, vals, blk_ptr, blk_dofs):
    """Dense A[dofs_b, dofs_b] for every block; returns (out_ptr, flat out)."""
    blk_ptr = np.ascontiguousarray(blk_ptr, dtype=np.int64)
    blk_dofs = np.ascontiguousarray(blk_dofs, dtype=np.int32)
    n = np.diff(blk_ptr)
    out_ptr = np.concatenate([[0], np.cumsum(n * n)]).astype(np.int64)
    out = np.empty(out_ptr[-1], dtype=np.float64)
    lib().alfi_host_extract_blocks(ctypes.c_int(d), _p(rowptr), _p(colidx), _p(vals), ctypes.c_int64(len(n)),
                                   _p(blk_ptr), _p(blk_dofs), _p(out_ptr), _p(out))
    return out_ptr, out


def interior_blocks(cell_nodes, g, vol, tensors, d, blk_nodes, num_nodes, nch, full_div=False):
    """K_II, D_II (nblk, m, m) of the coarse-cell interior dofs; children of block b are cells b*nch .. b*nch+nch-1."""
    cn = np.ascontiguousarray(cell_nodes, dtype=np.int32)
    nloc = cn.shape[1]
    nblk, mn = blk_nodes.shape
    m = mn * d
    blk_local = np.full(num_nodes, -1, dtype=np.int32)
    blk_local[blk_nodes.ravel()] = np.tile(np.arange(mn, dtype=np.int32), nblk)
    g = np.ascontiguousarray(g, dtype=np.float64)
    vol = np.ascontiguousarray(vol, dtype=np.float64)
    S, bI = (np.ascontiguousarray(tensors[k], dtype=np.float64) for k in ("S", "bI"))
    K = np.empty((nblk, m, m))
    D = np.empty((nblk, m, m))
    lib().alfi_host_interior_blocks(ctypes.c_int64(nblk), ctypes.c_int(nch), ctypes.c_int(nloc), ctypes.c_int(d),
                                    _p(cn), _p(g), _p(vol), _p(S), _p(bI), _p(blk_local), ctypes.c_int(m), _p(K), _p(D),
                                    ctypes.c_int(1 if full_div else 0))
    return K, D


def bsr_transpose(nbrows, nbcols, bs, rowptr, colidx, vals):
    rowptr_t = np.empty(nbcols + 1, dtype=np.int32)
    colidx_t = np.empty(colidx.shape[0], dtype=np.int32)
    vals_t = np.empty_like(vals)
    lib().alfi_host_bsr_transpose(ctypes.c_int64(nbrows), ctypes.c_int64(nbcols), ctypes.c_int(bs), _p(rowptr),
                                  _p(colidx), _p(vals), _p(rowptr_t), _p(colidx_t), _p(vals_t))
    return rowptr_t, colidx_t, vals_t
