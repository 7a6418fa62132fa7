"""Burman interior-penalty stabilisation of the Scott-Vogelius pair (alfi/stabilisation.py:139-162, set up in
alfi/solver.py:226-228 with h = problem.mesh_size(u, "facet"), added as ``advect * form(u, v)``, solver.py:233-234):

    R_B(u; v) = sum over interior facets F of  c_F beta_F(u) int_F jump(grad u, n) . jump(grad v, n) ds,
    c_F = 0.5 weight avg(h)^2   (h = FacetArea in 2-D, sqrt(FacetArea) in 3-D: h^2 = |F|^2 resp. |F|),
    beta_F(u) = |F|^-1 int_F sqrt(u.u + 1e-10) ds,   jump(grad u, n) = (grad u|K+ - grad u|K-) n+.

The wind is the state itself, so the Newton linearisation (UFL differentiates through facet_avg) has two parts:

    DR_B[du](v) = c_F beta_F int_F J(du).J(v)  +  c_F (|F|^-1 int_F u.du / sqrt(u.u + 1e-10)) int_F J(u).J(v).

Per facet the union of the two cells' nodes (9 for [P2]^2, 16 for [P3]^2, 30 for [P3]^3; K+'s nodes first) carries the jumps of the
normal derivatives at the points of an EXACT facet rule (S_F = int_F [d_n phi_a][d_n phi_b] is a polynomial of degree
2(k-1) on F: n = k points per direction); beta_F and the derivative weights m_(b,j) = |F|^-1 int_F phi_b u_j / sqrt(u.u +
1e-10) are not polynomial and use the rule NONLINEAR_RULE below (degree 2k + 2, UFL's estimate for sqrt of a degree-2k
argument).  With g_(a,i) = sum_b S_F[a][b] u_(b,i):

    residual (a, i)             += c_F beta_F g_(a,i)
    Jacobian ((a, i), (b, j))   += c_F beta_F S_F[a][b] delta_ij + c_F g_(a,i) m_(b,j)     (m: b on F only)

The host pass (csrc/host_assemble.cpp: alfi_host_burman) and the device pass (kernels_assemble.hip: alfi_level_burman)
take the same tables and the same contributor lists; every entry is summed by one thread in list order (no atomics)."""
import numpy as np

from . import _hostlib
from .elements import simplex_quadrature

DEFAULT_WEIGHT = 3e-3           # stabilisation.py:141-143 (the run lines of the reference pass 5e-3)
EPS = 1e-10                     # sqrt(u.u + 1e-10), stabilisation.py:159


def facet_rule(dim, n):
    """Rule on the reference facet of a dim-dimensional simplex, n points per direction (exact to degree 2n - 1):
    barycentric coordinates w.r.t. the facet's vertices (npts, dim) and weights summing to 1."""
    if dim == 2:
        x, w = np.polynomial.legendre.leggauss(n)
        x = 0.5 * (x + 1.0)
        return np.stack([1.0 - x, x], axis=1), w / w.sum()
    return simplex_quadrature(2, n)


def exact_rule_points(k):
    """n per direction of the rule that integrates S_F (degree 2(k-1)) exactly."""
    return max(1, k)


def nonlinear_rule_points(k):
    """NONLINEAR_RULE: n = k + 2 per direction, exact to degree 2k + 3 >= 2k + 2 (the degree UFL estimates for
    sqrt(u.u + eps) with u of degree k); shared by host, device and tests/burman_restatement.py."""
    return k + 2


class FacetTable(object):
    """Interior facets of a level (built once per hierarchy):
    union (nf, nu) int32     nodes of K+ (the cell of lower number) then the nodes of K- off the facet
    cfg (nf,) int32          configuration of K+ (which cell vertex is opposite F and how F's vertices map to the cell's)
    cells (nf, 2)            K+, K-;  area (nf,) |F|;  normal (nf, d) unit normal out of K+
    J (nf, nqs, nu)          jump of the normal derivative of every union basis function at the exact-rule points
    coef (nf,)               0.5 avg(h)^2 (times the weight at call time)
    ws (nqs,), wn (nqn,)     weights of the exact / nonlinear rule, summing to 1
    phin (ncfg, nqn, nloc)   K+'s basis at the nonlinear-rule points, zero for nodes off the facet
    onf (ncfg, nloc) uint8   K+'s local node lies on F"""

    def __init__(self, V):
        mesh, el, d = V.mesh, V.element, V.dim
        k = el.degree
        nloc = V.cell_nodes.shape[1]
        nfc = d + 1
        cf = mesh.cell_facets.ravel()
        order = np.argsort(cf, kind="stable")
        srt = cf[order]
        idx = np.flatnonzero(srt[:-1] == srt[1:])
        fid = srt[idx]
        kp, km = order[idx] // nfc, order[idx + 1] // nfc
        self.facet_ids = fid.astype(np.int64)
        self.cells = np.stack([kp, km], axis=1).astype(np.int64)
        nf = fid.shape[0]
        self.nf, self.d, self.nloc, self.k = nf, d, nloc, k
        fv = mesh.facets[fid]                                              # (nf, d) sorted global vertices of F
        cn_p, cn_m = V.cell_nodes[kp].astype(np.int64), V.cell_nodes[km].astype(np.int64)
        match = cn_m[:, :, None] == cn_p[:, None, :]                       # (nf, nloc-, nloc+)
        shared = match.any(axis=2)
        nsh = shared.sum(axis=1)
        assert nf == 0 or (nsh.min() == nsh.max()), "facets with differing numbers of shared nodes"
        nshared = int(nsh[0]) if nf else 0
        nu = 2 * nloc - nshared
        self.nu = nu
        upos = np.where(shared, match.argmax(axis=2), nloc + np.cumsum(~shared, axis=1) - 1)    # K- local node -> union
        union = np.empty((nf, nu), dtype=np.int64)
        union[:, :nloc] = cn_p
        rows = np.repeat(np.arange(nf), nloc)
        union[rows[~shared.ravel()], upos[~shared]] = cn_m[~shared]
        self.union = np.ascontiguousarray(union, dtype=np.int32)
        g, vol = mesh.cell_geometry()

        def side(K):
            cv = mesh.cells[K].astype(np.int64)                            # (nf, d+1)
            inf = cv[:, :, None] == fv[:, None, :]                        # (nf, d+1, d)
            opp = np.argmin(inf.any(axis=2), axis=1)
            pos = inf.argmax(axis=1)                                       # (nf, d): cell vertex of facet vertex t
            key = (pos * (d + 1) ** np.arange(d)).sum(axis=1)
            return opp, pos, key
        opp_p, pos_p, key_p = side(kp)
        opp_m, pos_m, key_m = side(km)
        gop = g[kp, opp_p]                                                 # grad lambda_opp of K+: points into K+
        gl = np.linalg.norm(gop, axis=1)
        self.normal = -gop / gl[:, None]
        self.area = d * vol[kp] * gl
        self.coef = 0.5 * (self.area ** 2 if d == 2 else self.area)
        mu_s, ws = facet_rule(d, exact_rule_points(k))
        mu_n, wn = facet_rule(d, nonlinear_rule_points(k))
        self.ws, self.wn = ws, wn
        nqs, nqn = len(ws), len(wn)
        keys = np.unique(np.concatenate([key_p, key_m]))

        def lam_of(pos, mu):
            lam = np.zeros((mu.shape[0], d + 1))
            for t in range(d):
                lam[:, pos[t]] = mu[:, t]
            return lam
        tab_s, tab_n = {}, {}
        for key in keys:
            pos = [(key // (d + 1) ** t) % (d + 1) for t in range(d)]
            tab_s[key] = el.tabulate(lam_of(pos, mu_s))[1]                # (nqs, nloc, d+1)
            tab_n[key] = el.tabulate(lam_of(pos, mu_n))[0]                # (nqn, nloc)
        J = np.zeros((nf, nqs, nu))
        for key in keys:
            for K, kk, sign in ((kp, key_p, 1.0), (km, key_m, -1.0)):
                sel = np.flatnonzero(kk == key)
                if sel.size == 0:
                    continue
                gn = np.einsum("fix,fx->fi", g[K[sel]], self.normal[sel])  # grad lambda_i . n
                dn = np.einsum("qai,fi->fqa", tab_s[key], gn)              # (f, q, nloc)
                if sign > 0:
                    J[sel, :, :nloc] += dn
                else:
                    np.add.at(J, (sel[:, None, None], np.arange(nqs)[None, :, None], upos[sel][:, None, :]), -dn)
        self.J = J
        cfg_keys, self.cfg = np.unique(key_p, return_inverse=True)
        self.cfg = self.cfg.astype(np.int32)
        onf_f = match.any(axis=1)                                          # (nf, nloc+): K+ node shared with K-
        ncfg = len(cfg_keys)
        self.phin = np.zeros((ncfg, nqn, nloc))
        self.onf = np.zeros((ncfg, nloc), dtype=np.uint8)
        for c, key in enumerate(cfg_keys):
            sel = np.flatnonzero(self.cfg == c)
            on = onf_f[sel[0]]
            assert (onf_f[sel] == on).all()
            self.onf[c] = on
            self.phin[c] = tab_n[key] * on[None, :]

    def subset(self, facets, union):
        """The table of the facets ``facets`` (indices into this table, ascending) with their union renumbered to ``union``
        (len(facets), nu): the rank-local table of a partitioned level (alfi_amd.dist.FacetPart).  The per-configuration
        tables are shared."""
        t = object.__new__(FacetTable)
        t.__dict__.update(self.__dict__)
        facets = np.asarray(facets, dtype=np.int64)
        for name in ("facet_ids", "cells", "normal", "area", "coef", "J", "cfg"):
            setattr(t, name, getattr(self, name)[facets])
        t.union = np.ascontiguousarray(union, dtype=np.int32)
        assert t.union.shape == (facets.size, self.nu)
        t.nf = int(facets.size)
        return t

    def pairs(self):
        """(rows, cols) node pairs the facets couple: what the level graph gains with facet coupling."""
        u = self.union.astype(np.int64)
        return np.repeat(u, self.nu, axis=1).ravel(), np.tile(u, (1, self.nu)).ravel()

    def contributors(self, rowptr, colidx, nnode, partial=False):
        """Matrix lists: (bptr int64 (nnzb+1), bfac int32, bab uint16 = a * nu + b) for every BSR block, facets ascending;
        residual lists: (nptr int64 (nnode+1), nfac int32, na uint16) for every node.  partial: the union may hold nodes
        >= nnode (a rank-local table, its union in the numbering of the rank's state vector): only the pairs whose row and
        column are below nnode -- rows and columns of the rank's localised sparsity -- and the nodes below nnode are listed."""
        nu, nf = self.nu, self.nf
        rowptr = np.asarray(rowptr, dtype=np.int64)
        colidx = np.asarray(colidx, dtype=np.int64)
        nnzb = colidx.shape[0]
        bkey = np.repeat(np.arange(nnode, dtype=np.int64), np.diff(rowptr)) * nnode + colidx
        bord = None
        if nnzb and not (np.diff(bkey) > 0).all():
            # (a localised sparsity: columns in local numbering are not ascending inside a row)
            assert partial, "unsorted block rows"
            bord = np.argsort(bkey, kind="stable")
            bkey = bkey[bord]
            assert (np.diff(bkey) > 0).all(), "repeated blocks"
        r, c = self.pairs()
        pair = np.arange(nf * nu * nu, dtype=np.int64)
        if partial:
            keep = (r < nnode) & (c < nnode)
            r, c, pair = r[keep], c[keep], pair[keep]
        else:
            assert nf == 0 or int(self.union.max()) < nnode, "union node beyond the level's nodes"
        key = r * nnode + c
        blk = np.searchsorted(bkey, key)
        if key.size and (blk.max() >= nnzb or (bkey[np.minimum(blk, nnzb - 1)] != key).any()):
            raise ValueError("the level graph lacks facet-coupled blocks (build the hierarchy with facet_coupling=True)")
        if bord is not None:
            blk = bord[blk]
        o = np.argsort(blk, kind="stable")
        bptr = np.zeros(nnzb + 1, dtype=np.int64)
        np.cumsum(np.bincount(blk, minlength=nnzb), out=bptr[1:])
        bfac = (pair[o] // (nu * nu)).astype(np.int32)
        bab = (pair[o] % (nu * nu)).astype(np.uint16)
        un = self.union.ravel().astype(np.int64)
        slot = np.arange(un.size, dtype=np.int64)
        if partial:
            slot = slot[un < nnode]
            un = un[slot]
        o2 = np.argsort(un, kind="stable")
        nptr = np.zeros(nnode + 1, dtype=np.int64)
        np.cumsum(np.bincount(un, minlength=nnode), out=nptr[1:])
        nfac = (slot[o2] // nu).astype(np.int32)
        na = (slot[o2] % nu).astype(np.uint16)
        return (bptr, bfac, bab), (nptr, nfac, na)


def facet_coupled_graph(cell_nodes, num_nodes, table):
    """Node graph of the cells united with the facet pairs: ``_hostlib.node_graph`` over the cells followed by one
    "two-cell" node list per interior facet."""
    cn = np.asarray(cell_nodes, dtype=np.int32)
    nloc, nu = cn.shape[1], table.nu
    # the facet lists are wider than a cell: the cells are padded with copies of their first node (node_graph drops repeats)
    wide = np.concatenate([np.concatenate([cn, np.repeat(cn[:, :1], nu - nloc, axis=1)], axis=1), table.union], axis=0)
    return _hostlib.node_graph(wide, num_nodes)


class HostBurman(object):
    """The host pass over one level: residual contribution and / or Newton linearisation (alfi_host_burman)."""

    def __init__(self, L, table=None):
        self.table = table if table is not None else L.facets
        V = L.V
        self.lists = self.table.contributors(L.A.rowptr, L.A.colidx, V.num_nodes)

    def __call__(self, U, weight, vals=None, F=None, beta=None):
        _hostlib.burman(self.table, U, weight, self.lists, vals=vals, F=F, beta=beta)


def patch_cells(V, patch_nodes):
    """The cells of a patch for PCPATCH's facet rule: the cells holding one of its nodes (the cells in the star of a patch point
    that carries a free dof)."""
    hit = np.zeros(V.num_nodes, dtype=bool)
    hit[patch_nodes] = True
    return np.flatnonzero(hit[V.cell_nodes].any(axis=1))


def patch_facet_corrections(V, table, patch_ptr, patch_dofs):
    """PCPATCH's interior-facet rule (Firedrake's PatchPC: PETSc PCPatchCreateCellPatchFacets collects for a patch the interior
    facets whose two cells both belong to it; only those are integrated into the patch's matrix).  The global sub-block A[P, P]
    also holds, for every facet F with ONE cell K in the patch, F's K-side term c_F beta_F S_F on K's patch nodes -- F's own
    nodes and the other cell's nodes are not patch dofs (any cell holding a patch node is a patch cell), so neither the other
    S_F blocks nor the g (x) m columns (nodes on F) reach the patch; asserted here.  Returns the lists of
    alfi_patches_set_facet_correction: per patch-local row node (rows numbered patch_ptr[p] / d + i) the entries (col, facet,
    s = c_F |F| sum_q ws_q J_qa J_qb), ordered by column node then facet."""
    d, nu, nloc = V.dim, table.nu, table.nloc
    patch_ptr = np.asarray(patch_ptr, dtype=np.int64)
    patch_dofs = np.asarray(patch_dofs, dtype=np.int64)
    assert (patch_ptr % d == 0).all()
    ncell = V.mesh.num_cells
    # facets of every cell, with the cell's side
    fc = np.concatenate([table.cells[:, 0], table.cells[:, 1]])
    fs = np.concatenate([np.zeros(table.nf, dtype=np.int64), np.ones(table.nf, dtype=np.int64)])
    ff = np.concatenate([np.arange(table.nf), np.arange(table.nf)])
    order = np.argsort(fc, kind="stable")
    cptr = np.zeros(ncell + 1, dtype=np.int64)
    np.cumsum(np.bincount(fc, minlength=ncell), out=cptr[1:])
    cfac, cside = ff[order], fs[order]
    Sfull = np.einsum("q,fqa,fqb->fab", table.ws, table.J, table.J) * (table.coef * table.area)[:, None, None]
    rows_ptr, cols, facs, svals = [0], [], [], []
    local = np.full(V.num_nodes, -1, dtype=np.int64)
    for p in range(len(patch_ptr) - 1):
        nodes = patch_dofs[patch_ptr[p]:patch_ptr[p + 1]:d] // d
        local[nodes] = np.arange(nodes.size)
        cells = patch_cells(V, nodes)
        inside = np.zeros(ncell, dtype=bool)
        inside[cells] = True
        ent = [[] for _ in range(nodes.size)]
        for K in cells:
            for f, side in zip(cfac[cptr[K]:cptr[K + 1]], cside[cptr[K]:cptr[K + 1]]):
                other = table.cells[f, 1 - side]
                if inside[other]:
                    continue                                  # both cells in the patch: PCPATCH integrates the facet
                un = table.union[f].astype(np.int64)
                loc = local[un]
                kpos = np.flatnonzero(np.isin(un, V.cell_nodes[K]))
                assert (loc[np.setdiff1d(np.arange(nu), kpos)] < 0).all(), "a node off K is a patch dof"
                assert (loc[kpos[np.isin(un[kpos], V.cell_nodes[other])]] < 0).all(), "a node on the facet is a patch dof"
                for a in kpos[loc[kpos] >= 0]:
                    for b in kpos[loc[kpos] >= 0]:
                        ent[loc[a]].append((loc[b], f, Sfull[f, a, b]))
        for e in ent:
            e.sort(key=lambda t: (t[0], t[1]))
            cols.extend(t[0] for t in e)
            facs.extend(t[1] for t in e)
            svals.extend(t[2] for t in e)
            rows_ptr.append(rows_ptr[-1] + len(e))
        local[nodes] = -1
    return (np.array(rows_ptr, dtype=np.int64), np.array(cols, dtype=np.int32), np.array(facs, dtype=np.int32),
            np.array(svals, dtype=np.float64))
