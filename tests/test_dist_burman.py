"""Burman terms on partitioned levels, on the host (-m "not gpu"): every rank's facets (alfi_amd.dist.FacetPart) give its rows
and residual entries of the global host pass bit for bit, cover every facet that reaches a local row, and carry PCPATCH's
facet rule for its owned patches in local numbering."""
import functools

import numpy as np
import pytest

from alfi_amd import _hostlib
from alfi_amd.burman import patch_facet_corrections
from alfi_amd.dist import FacetPart, build_parts, choose_splits, local_host_operator, localize
from alfi_amd.problem import ThreeDimLidDrivenCavityProblem, TwoDimLidDrivenCavityProblem
from alfi_amd.sv import build_sv_hierarchy

WEIGHT = 5e-3 * 0.7


@functools.lru_cache(maxsize=None)
def _hierarchy(case):
    if case == "2d-P2":
        return build_sv_hierarchy(TwoDimLidDrivenCavityProblem(4), 2, 2, Re=0.0, facet_coupling=True)
    return build_sv_hierarchy(ThreeDimLidDrivenCavityProblem(1), 1, 3, Re=0.0, facet_coupling=True)


def _rank_levels(case, world):
    """(global levels, [(rank, local level)] for every rank and every level it owns rows of)."""
    levels, transfers = _hierarchy(case)
    splits = choose_splits(levels, world, min_dofs=1)
    out = []
    for rank in range(world):
        parts = build_parts(levels, transfers, splits, rank, exchange_lists=None)
        llev, _, _ = localize(levels, transfers, parts)
        out.extend((rank, LL) for LL in llev if LL.part.nb_own > 0)
    return levels, out


def _global_blocks(L, rows, cols):
    """Index of the global block (rows[i], cols[i]) of level L's operator (asserted present)."""
    n = L.V.num_nodes
    gkey = np.repeat(np.arange(n, dtype=np.int64), np.diff(L.A.rowptr)) * n + L.A.colidx
    key = rows * n + cols
    idx = np.searchsorted(gkey, key)
    assert (idx < gkey.size).all() and (gkey[np.minimum(idx, gkey.size - 1)] == key).all()
    return idx


CASES = [pytest.param("2d-P2", 2, id="2d-P2-2ranks"), pytest.param("2d-P2", 3, id="2d-P2-3ranks"),
         pytest.param("3d-P3", 2, id="3d-P3-2ranks"), pytest.param("3d-P3", 3, id="3d-P3-3ranks")]


@pytest.mark.parametrize("case,world", CASES)
def test_rank_host_pass_equals_global_rows(case, world):
    """Owned rows complete, ghost rows on their local columns, every local residual entry and beta_F of the rank's facets:
    BITWISE equal to the global host pass -- the rank's facets are a subset in ascending global order, so every block and every
    node sums the same contributors in the same order."""
    levels, ranks = _rank_levels(case, world)
    seen = set()
    for rank, LL in ranks:
        L, part = levels[LL.level], LL.part
        d, n = L.bs, L.V.num_nodes
        U = np.random.default_rng(LL.level + 10 * rank).standard_normal((n, d))
        gvals, gF, gbeta = np.zeros((L.A.colidx.size, d, d)), np.zeros(n * d), np.empty(L.facets.nf)
        _hostlib.burman(L.facets, U, WEIGHT, L.facets.contributors(L.A.rowptr, L.A.colidx, n), vals=gvals, F=gF, beta=gbeta)
        fp = FacetPart(L.V, L.facets, part)
        assert np.array_equal(fp.state_nodes[:part.nb_loc], part.nodes)
        assert np.unique(fp.state_nodes).size == fp.state_nodes.size
        assert fp.table.union.max() < fp.state_nodes.size
        assert np.array_equal(fp.state_nodes[fp.table.union], L.facets.union[fp.facets])
        lvals, lF, lbeta = np.zeros((LL.A.colidx.size, d, d)), np.zeros(part.nb_loc * d), np.empty(fp.table.nf)
        fp.host(LL.A, U[fp.state_nodes], WEIGHT, vals=lvals, F=lF, beta=lbeta)
        rows = np.repeat(part.nodes, np.diff(LL.A.rowptr))
        idx = _global_blocks(L, rows, part.nodes[LL.A.colidx])
        assert np.array_equal(lvals, gvals[idx])
        # the owned rows are complete: as many blocks as the global rows
        assert LL.A.rowptr[part.nb_own] == sum(L.A.rowptr[g + 1] - L.A.rowptr[g] for g in part.own_nodes)
        assert np.array_equal(lF.reshape(-1, d), gF.reshape(-1, d)[part.nodes])
        assert np.array_equal(lbeta, gbeta[fp.facets])
        # the Burman part is really there on the rank's rows
        assert np.abs(lvals).max() > 0.0 and np.abs(lF).max() > 0.0
        seen.add(rank)
    assert seen == set(range(world))


@pytest.mark.parametrize("case,world", CASES)
def test_rank_facets_cover_local_rows(case, world):
    """Every facet with a union node among the rank's local nodes (owned or ghost) is one of its facets; facets reaching an
    owned node reach local nodes only."""
    levels, ranks = _rank_levels(case, world)
    for rank, LL in ranks:
        L, part = levels[LL.level], LL.part
        fp = FacetPart(L.V, L.facets, part)
        local = np.zeros(L.V.num_nodes, dtype=bool)
        local[part.nodes] = True
        reach = np.flatnonzero(local[L.facets.union].any(axis=1))
        assert np.isin(reach, fp.facets).all(), (rank, LL.level)
        own = np.zeros(L.V.num_nodes, dtype=bool)
        own[part.own_nodes] = True
        assert local[L.facets.union[own[L.facets.union].any(axis=1)]].all()
        assert np.array_equal(fp.facets, np.unique(fp.facets))


def _corrections_by_node(ptr, col, fac, s, patch_ptr, node_of_dof, d):
    """{(patch index, row node, column node, facet): s} in global numbering."""
    out = {}
    for p in range(len(patch_ptr) - 1):
        nodes = node_of_dof[patch_ptr[p]:patch_ptr[p + 1]:d]
        r0 = patch_ptr[p] // d
        for i in range(nodes.size):
            for q in range(ptr[r0 + i], ptr[r0 + i + 1]):
                out[(p, int(nodes[i]), int(nodes[col[q]]), int(fac[q]))] = float(s[q])
    return out


@pytest.mark.parametrize("case,world", [CASES[0], CASES[2]])
def test_patch_facet_corrections_in_local_numbering(case, world):
    """PCPATCH's facet rule for a rank's owned patches (FacetPart.patch_facet_corrections: local rows / columns, the rank's
    facet ids), mapped back to global numbering, equals the rule of the same patches on the global level."""
    levels, ranks = _rank_levels(case, world)
    checked = 0
    for rank, LL in ranks:
        if LL.level == 0:
            continue
        L, part, d = levels[LL.level], LL.part, LL.bs
        fp = FacetPart(L.V, L.facets, part)
        ptr, col, fac, s = fp.patch_facet_corrections(L.V, L.facets, LL)
        assert fac.dtype == np.int32 and (fac >= 0).all() and (fac < fp.table.nf).all()
        loc = _corrections_by_node(ptr, col, fp.facets[fac], s, LL.patch_ptr, part.nodes[LL.patch_dofs // d], d)
        # the same patches, as the global level lists them
        gptr = [0]
        gdofs = []
        for pid in LL.patch_ids:
            dofs = L.patch_dofs[L.patch_ptr[pid]:L.patch_ptr[pid + 1]]
            gdofs.append(dofs)
            gptr.append(gptr[-1] + dofs.size)
        gptr = np.array(gptr, dtype=np.int64)
        gdofs = np.concatenate(gdofs)
        g = patch_facet_corrections(L.V, L.facets, gptr, gdofs)
        glob = _corrections_by_node(*g, gptr, gdofs // d, d)
        assert loc == glob, (rank, LL.level)
        checked += len(loc)
    assert checked > 0


@pytest.mark.parametrize("case,world", [CASES[1], CASES[2]])
def test_rank_host_operator_equals_global_rows(case, world):
    """local_host_operator (the rank's rows of the ALFI_DEVICE_ASSEMBLY=0 path: cells, then the rank's facets, then the
    boundary conditions) against the global host assembly of the same rows, Burman term included."""
    levels, ranks = _rank_levels(case, world)
    nu, gamma, adv = 0.05, 1e4, 1.0
    for rank, LL in ranks:
        L, part = levels[LL.level], LL.part
        V, d = L.V, L.bs
        wind = np.random.default_rng(3 + rank).standard_normal((V.num_nodes, d))
        g, vol = V.mesh.cell_geometry()
        ref = _hostlib.assemble_bsr(V.cell_nodes, g, vol, V.element.reference_tensors(), d, L.A.rowptr, L.A.colidx, nu=nu,
                                    gamma=0.0, gamma_full=gamma, adv=adv, wind=wind)
        beta_g = np.empty(L.facets.nf)
        _hostlib.burman(L.facets, wind, adv * WEIGHT, L.facets.contributors(L.A.rowptr, L.A.colidx, V.num_nodes), vals=ref,
                        beta=beta_g)
        _hostlib.apply_bc_bsr(V.num_nodes, d, L.A.rowptr, L.A.colidx, ref, np.repeat(V.bc_node_mask, d))
        fp = FacetPart(V, L.facets, part)
        A, beta = local_host_operator(L, part, fp, nu, gamma, adv, wind, WEIGHT)
        assert np.array_equal(A.rowptr, LL.A.rowptr) and np.array_equal(A.colidx, LL.A.colidx)
        idx = _global_blocks(L, np.repeat(part.nodes, np.diff(A.rowptr)), part.nodes[A.colidx])
        # (the cell terms of a row subset are summed by the row-map pass of the generator: equal up to rounding)
        assert np.abs(A.vals - ref[idx]).max() <= 1e-13 * np.abs(ref).max()
        assert np.array_equal(beta, beta_g[fp.facets])
