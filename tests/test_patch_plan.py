"""The host planners behind alfi_patches_set, alfi_patches_set_groups and alfi_patches_set_multiplicative (csrc/patch_plan.h)
through the exports of libalfi_host.so (_hostlib.plan_patch_layout / plan_condensed / plan_sweep).  No GPU.

* Every table against tests/golden/patch_plan_{a,b,c}.npz.  The fixtures are the tables of the commit BEFORE the planners
  left csrc/api_patches.hip: its loops, text unchanged, compiled into a host program with the device calls replaced by host
  memory, every uploaded array written out (keys "<planner>.<table>").  Cases: tests/patch_plan_cases.py.
* The condensed tables by their meaning: the block factorisation applied through them equals np.linalg.solve.  Tolerance:
  1e-8 in the max norm relative to the reference, the bound of the condensed-against-dense comparison on the device
  (tests/test_gpu_condensed.py, tests/test_gpu_star_condense.py) -- here NumPy FP64 on the same patches.
* The schedule by its meaning: predecessor counts against a brute-force count, and Gauss-Seidel in any order the
  dependencies allow against list order, bit for bit.
* Every refusal with its code (ALFI_E_ARG = -2) and text."""
import os

import numpy as np
import pytest

from tests.patch_plan_cases import case, plans

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
E_ARG = -2
TOL = 1e-8


def relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def ldim(rows):                                    # cond_ldim, csrc/cond_layout.h
    return (rows + 1) & ~1


def pairs(rows):                                   # cond_pairs
    return (rows + 1) // 2


def group_doubles(m, sc):                          # cond_group_doubles
    return ldim(m) * m + ldim(sc) * m + ldim(m) * sc


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_every_table_equals_the_one_the_api_functions_built(name):
    L, groups, iterset = case(name)
    got = plans(name)
    ref = np.load(os.path.join(GOLDEN, "patch_plan_%s.npz" % name))
    keys = sorted(p + "." + k for p in got for k in got[p])
    assert keys == sorted(ref.files)
    for key in keys:
        p, k = key.split(".")
        v = got[p][k]
        if isinstance(v, np.ndarray):
            assert v.dtype == ref[key].dtype and np.array_equal(v, ref[key]), key
        else:
            assert v == int(ref[key]), key
    sizes = np.diff(L.patch_ptr)
    grouped = sum(bool((groups[L.patch_ptr[p]:L.patch_ptr[p + 1]] >= 0).any()) for p in range(len(sizes)))
    cd, sw = got["cond"], got["sweep"]
    if name == "b":
        assert len(sizes) == 125 and sizes.max() == 153 and grouped == 81
        full = np.flatnonzero(sizes == 153)
        assert all(cd["g_m"][cd["gptr"][p]:cd["gptr"][p + 1]].tolist() == [15] * 6 for p in full)
    if name == "c":
        assert len(sizes) == 27 and sizes.max() == 1599
        assert cd["max_pairs"] > 256 and (np.diff(cd["gcptr"]) > 1).any() and (np.diff(cd["chptr"]) > 1).any()
        assert sw["big"] == 1 and len(sw["rowtab"]) == 0
    else:
        assert sw["big"] == 0 and len(sw["rowtab"]) == len(sizes) * 64 * 3


# ---- the condensed plan ------------------------------------------------------------------------------------------------------
def _patch_factors(cd, Ac, p):
    """X_g, B_g, W_g of every group of patch p stored in a `mat` buffer the way CondDev::mat is ([X | B | W], column-major,
    even leading dimensions, at g_mat), and inv(Sigma) dense; Ac: the patch matrix in the condensed order."""
    n = Ac.shape[0]
    nI = int(cd["p_nI"][p])
    s = n - nI
    g0, g1 = int(cd["gptr"][p]), int(cd["gptr"][p + 1])
    base = int(cd["g_mat"][g0]) if g1 > g0 else 0
    mat = np.zeros(sum(group_doubles(int(cd["g_m"][g]), int(cd["g_sc"][g])) for g in range(g0, g1)))
    Sigma = Ac[nI:, nI:].copy()
    for g in range(g0, g1):
        m, sc, o = int(cd["g_m"][g]), int(cd["g_sc"][g]), int(cd["g_off"][g])
        Sg = nI + cd["sidx"][cd["g_sidx"][g]:cd["g_sidx"][g] + sc]
        # everything the group touches outside itself lies in S_g
        others = np.setdiff1d(np.arange(n), np.concatenate([np.arange(o, o + m), Sg]))
        assert not Ac[o:o + m, others].any() and not Ac[others, o:o + m].any()
        X = np.linalg.inv(Ac[o:o + m, o:o + m])
        B = Ac[Sg, o:o + m]
        # (W by LU, not as the product X A[g, S_g]: the product's residual A_gg W - A[g, S_g] is cond(A_gg) eps large and
        # inv(Sigma) amplifies it -- 3e-5 against np.linalg.solve on the stars of case b, 7e-11 this way)
        W = np.linalg.solve(Ac[o:o + m, o:o + m], Ac[o:o + m, Sg])
        Sigma[np.ix_(Sg - nI, Sg - nI)] -= B @ W
        at = int(cd["g_mat"][g]) - base
        assert at + group_doubles(m, sc) <= len(mat)
        ldm, ldsc = ldim(m), ldim(sc)
        for blk, ld, a in ((X, ldm, at), (B, ldsc, at + ldm * m), (W, ldm, at + ldm * m + ldsc * m)):
            v = mat[a:a + ld * blk.shape[1]].reshape(blk.shape[1], ld)        # column-major: [column][row]
            assert not v.any()                                                # nobody wrote here before: no overlap
            v[:, :blk.shape[0]] = blk.T
    return mat, base, np.linalg.inv(Sigma) if s else np.zeros((0, 0))


def _rows(cd, mat, base, g, which, row):
    """row `row` of X_g (which 0), B_g (1) or W_g (2) read from the mat buffer"""
    m, sc = int(cd["g_m"][g]), int(cd["g_sc"][g])
    ldm, ldsc = ldim(m), ldim(sc)
    at = int(cd["g_mat"][g]) - base
    off, ld, ncol = ((at, ldm, m), (at + ldm * m, ldsc, m), (at + ldm * m + ldsc * m, ldm, sc))[which]
    return mat[off:off + ld * ncol].reshape(ncol, ld)[:, row]


@pytest.mark.parametrize("name", ["a", "b"])
def test_block_factorisation_through_the_condensed_tables_solves_the_patch_systems(name):
    L, groups, _ = case(name)
    cd, lay = plans(name)["cond"], plans(name)["layout"]
    pp, pd = np.asarray(L.patch_ptr), np.asarray(L.patch_dofs)
    S = L.A.to_scipy().tocsr()
    x = np.random.default_rng(11).standard_normal(L.n)
    stage = {form: np.zeros(lay["stage_len"]) for form in ("patch", "chunk")}
    ubuf = {form: np.full(int(cd["uptr"][-1]), np.nan) for form in ("patch", "chunk")}
    worst = 0.0
    for p in range(len(pp) - 1):
        off, n = int(pp[p]), int(pp[p + 1] - pp[p])
        slot = cd["slot"][off:off + n]
        assert np.array_equal(np.sort(slot), np.arange(n)) and np.array_equal(cd["dofs"][off:off + n], pd[off + slot])
        dofs = pd[off:off + n]
        Ap = S[dofs][:, dofs].toarray()
        Ac = Ap[np.ix_(slot, slot)]
        mat, base, Sinv = _patch_factors(cd, Ac, p)
        nI, s = int(cd["p_nI"][p]), n - int(cd["p_nI"][p])
        assert s == cd["sptr"][p + 1] - cd["sptr"][p]
        xc = x[cd["dofs"][off:off + n]]
        g0 = int(cd["gptr"][p])
        ub, uo = int(cd["uptr"][p]), int(cd["uptr"][p + 1] - cd["uptr"][p])
        r0 = int(cd["sptr"][p])
        qb = int(cd["s_uptr"][r0])
        xp0, bp0 = int(cd["xp_ptr"][p]), int(cd["bp_ptr"][p])

        def front(form, xq, bq, t):
            """t = X x on the X pairs xq, then u = B t on the B pairs bq, into the row-sorted u buffer"""
            for k in xq:
                g = int(cd["xp_grp"][k])
                m, o = int(cd["g_m"][g]), int(cd["g_off"][g])
                for r in range(2 * (k - xp0 - int(cd["g_xp"][g])), min(2 * (k - xp0 - int(cd["g_xp"][g])) + 2, m)):
                    t[o + r] = _rows(cd, mat, base, g, 0, r) @ xc[o:o + m]
            for k in bq:
                g = int(cd["bp_grp"][k])
                m, sc, o = int(cd["g_m"][g]), int(cd["g_sc"][g]), int(cd["g_off"][g])
                for r in range(2 * (k - bp0 - int(cd["g_bp"][g])), min(2 * (k - bp0 - int(cd["g_bp"][g])) + 2, sc)):
                    ubuf[form][ub + cd["u_dst"][ub + cd["g_uoff"][g] + r]] = _rows(cd, mat, base, g, 1, r) @ t[o:o + m]

        def sigma(form):
            """y_S = inv(Sigma) (x_S - the contributions of every skeleton row, contiguous in the row-sorted buffer)"""
            rhs = xc[nI:].copy()
            for i in range(s):
                a, b = int(cd["s_uptr"][r0 + i]) - qb, int(cd["s_uptr"][r0 + i + 1]) - qb
                rhs[i] -= ubuf[form][ub + a:ub + b].sum()
            return Sinv @ rhs

        def back(form, xq, t, yS, sidx_of, stage_off):
            """y_g = t_g - W_g y_S[S_g] on the pairs xq, staged at the entry's slot"""
            for k in xq:
                g = int(cd["xp_grp"][k])
                m, sc, o = int(cd["g_m"][g]), int(cd["g_sc"][g]), int(cd["g_off"][g])
                for r in range(2 * (k - xp0 - int(cd["g_xp"][g])), min(2 * (k - xp0 - int(cd["g_xp"][g])) + 2, m)):
                    stage[form][stage_off + slot[o + r]] = t[o + r] - _rows(cd, mat, base, g, 2, r) @ yS[sidx_of(g)]

        # the per-patch form: xp_grp / g_xp, bp_grp / g_bp, u_dst, s_uptr, slot
        t = np.full(n, np.nan)
        front("patch", range(xp0, int(cd["xp_ptr"][p + 1])), range(bp0, int(cd["bp_ptr"][p + 1])), t)
        yS = sigma("patch")
        st = int(lay["stage_ptr"][p])
        back("patch", range(xp0, int(cd["xp_ptr"][p + 1])), t, yS,
             lambda g: cd["sidx"][cd["g_sidx"][g]:cd["g_sidx"][g] + cd["g_sc"][g]], st)
        stage["patch"][st + slot[nI:]] = yS
        # the chunked form: CondChunk ranges, the ubuf order, sidx0, stage_off
        chunks = cd["gc"][int(cd["gcptr"][p]):int(cd["gcptr"][p + 1])]
        t = np.full(n, np.nan)
        for c in chunks:
            assert (c["off"], c["ubase"], c["stage_off"], c["nI"], c["xp0"], c["bp0"]) == (off, ub, st, nI, xp0, bp0)
            tc = np.full(n, np.nan)                     # a chunk sees its own interior entries only
            front("chunk", range(c["xq0"], c["xq1"]), range(c["bq0"], c["bq1"]), tc)
            filled = np.flatnonzero(~np.isnan(tc))
            assert np.array_equal(filled, np.arange(c["e0"], c["e0"] + c["ne"]))
            t[filled] = tc[filled]
        yS = sigma("chunk")
        for c in chunks:
            lists = cd["sidx"][c["sidx0"]:c["sidx0"] + c["nu"]]             # the chunk's S_g lists, in the order of its u entries
            back("chunk", range(c["xq0"], c["xq1"]), t, yS,
                 lambda g: lists[cd["g_uoff"][g] - c["u0"]:cd["g_uoff"][g] - c["u0"] + cd["g_sc"][g]], int(c["stage_off"]))
        stage["chunk"][st + slot[nI:]] = yS
        assert not np.isnan(ubuf["patch"][ub:ub + uo]).any() and np.array_equal(ubuf["patch"][ub:ub + uo], ubuf["chunk"][ub:ub + uo])
        ref = np.linalg.solve(Ap, x[dofs])
        for form in ("patch", "chunk"):
            err = relerr(stage[form][st:st + n], ref)
            worst = max(worst, err)
            assert err < TOL, (p, form, err)
        assert g0 <= int(cd["gptr"][p + 1])
    print("case %s: worst error of the staged results against np.linalg.solve %.3e" % (name, worst))


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_invariants_of_the_condensed_tables(name):
    L, _, _ = case(name)
    cd = plans(name)["cond"]
    npatch = len(L.patch_ptr) - 1
    nbytes = np.zeros(npatch, dtype=np.int64)
    for p in range(npatch):
        g0, g1 = int(cd["gptr"][p]), int(cd["gptr"][p + 1])
        s = int(cd["sptr"][p + 1] - cd["sptr"][p])
        nbytes[p] = s * s + sum(group_doubles(int(cd["g_m"][g]), int(cd["g_sc"][g])) for g in range(g0, g1))
        # u_dst restricted to the patch is the inverse permutation of s_uidx
        ub, uo = int(cd["uptr"][p]), int(cd["uptr"][p + 1] - cd["uptr"][p])
        qb, qe = int(cd["s_uptr"][cd["sptr"][p]]), int(cd["s_uptr"][cd["sptr"][p + 1]])
        perm = cd["s_uidx"][qb:qe]
        assert qe - qb == uo == int(cd["g_sc"][g0:g1].sum()) and np.array_equal(np.sort(perm), np.arange(uo))
        assert np.array_equal(cd["u_dst"][ub + perm], np.arange(uo))
        # the chunks of the patch tile its groups without gap or overlap, each of <= 256 pairs of X / W and of B
        chunks = cd["gc"][int(cd["gcptr"][p]):int(cd["gcptr"][p + 1])]
        assert (len(chunks) > 0) == (g1 > g0)
        xq, bq, e, u = int(cd["xp_ptr"][p]), int(cd["bp_ptr"][p]), 0, 0
        for c in chunks:
            assert (c["xq0"], c["bq0"], c["e0"], c["u0"]) == (xq, bq, e, u)
            assert 0 < c["xq1"] - c["xq0"] <= 256 and 0 <= c["bq1"] - c["bq0"] <= 256
            g = np.unique(cd["xp_grp"][c["xq0"]:c["xq1"]])
            assert np.array_equal(g, np.arange(g[0], g[-1] + 1))                      # whole, consecutive groups
            assert c["xq1"] - c["xq0"] == sum(pairs(int(m)) for m in cd["g_m"][g])
            assert c["bq1"] - c["bq0"] == sum(pairs(int(sc)) for sc in cd["g_sc"][g])
            assert c["ne"] == cd["g_m"][g].sum() and c["nu"] == cd["g_sc"][g].sum() and c["sidx0"] == cd["g_sidx"][g[0]]
            xq, bq, e, u = int(c["xq1"]), int(c["bq1"]), e + int(c["ne"]), u + int(c["nu"])
        assert (xq, bq, e, u) == (int(cd["xp_ptr"][p + 1]), int(cd["bp_ptr"][p + 1]), int(cd["p_nI"][p]), uo)
        # sigma chunks: every 64 rows of the even-padded skeleton
        rows = cd["ch_row"][int(cd["chptr"][p]):int(cd["chptr"][p + 1])]
        assert np.array_equal(rows, np.arange(0, ldim(s), 64)) and (cd["ch_patch"][int(cd["chptr"][p]):int(cd["chptr"][p + 1])] == p).all()
    # the dispatch order: a permutation, by descending factor bytes, ties by index
    assert np.array_equal(cd["order"], np.array(sorted(range(npatch), key=lambda p: (-nbytes[p], p)), dtype=np.int32))
    assert cd["mat_doubles"] == nbytes.sum() - (np.diff(cd["sptr"]) ** 2).sum() and cd["ngroups"] == len(cd["g_m"])


# ---- the sweep schedule --------------------------------------------------------------------------------------------------------
def _patch_nodes(L, p):
    return np.asarray(L.patch_dofs[L.patch_ptr[p]:L.patch_ptr[p + 1]:L.bs]) // L.bs


def _closure(L, nodes):
    rp, ci = L.A.rowptr, L.A.colidx
    return np.unique(np.concatenate([ci[rp[i]:rp[i + 1]] for i in nodes]))


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_schedule_is_the_last_writer_relation_of_the_list_order(name):
    L, _, iterset = case(name)
    sw = plans(name)["sweep"]
    seq, wp, items = sw["seq"], sw["wave_ptr"], sw["items"]
    assert np.array_equal(np.sort(seq), np.sort(iterset)) and wp[0] == 0 and wp[-1] == len(seq) and (np.diff(wp) > 0).all()
    rev = [seq[wp[w]:wp[w + 1]] for w in range(len(wp) - 2, -1, -1)]
    assert np.array_equal(items, np.concatenate([seq] + rev)) and sw["nitems"] == len(items)
    N, nb = len(items), len(L.A.rowptr) - 1
    writes = np.zeros((N, nb), dtype=bool)
    for t in range(N):
        writes[t, _patch_nodes(L, items[t])] = True
    edges = set()
    for t in range(N):
        cols = _closure(L, _patch_nodes(L, items[t]))
        sub = writes[:t][:, cols]
        sub = sub[:, sub.any(axis=0)]                                           # the nodes t reads that an earlier item wrote
        pred = np.unique(t - 1 - np.argmax(sub[::-1], axis=0)) if sub.size else []   # ... and the last writer of each
        assert sw["pred0"][t] == len(pred), t
        edges |= {(int(f), t) for f in pred}
    sp = sw["succ_ptr"]
    assert sp[0] == 0 and sp[-1] == len(edges) and len(sp) == N + 1
    got = {(f, int(t)) for f in range(N) for t in sw["succ"][sp[f]:sp[f + 1]]}
    assert got == edges
    assert all(np.array_equal(sw["succ"][sp[f]:sp[f + 1]], np.sort(sw["succ"][sp[f]:sp[f + 1]])) for f in range(N))


@pytest.mark.parametrize("name", ["a", "b"])
def test_any_order_the_dependencies_allow_gives_the_bits_of_list_order(name):
    """What the persistent sweep kernel rests on: an item may run as soon as its predecessors have."""
    L, _, _ = case(name)
    sw = plans(name)["sweep"]
    items, pred0, sp, succ = sw["items"], sw["pred0"], sw["succ_ptr"], sw["succ"]
    S = L.A.to_scipy().tocsr()
    bs = L.bs
    work = {}
    for p in np.unique(items):
        rows = np.asarray(L.patch_dofs[L.patch_ptr[p]:L.patch_ptr[p + 1]])
        cols = (_closure(L, _patch_nodes(L, p))[:, None] * bs + np.arange(bs)).ravel()
        work[int(p)] = (rows, cols, S[rows][:, cols].toarray(), np.linalg.inv(S[rows][:, rows].toarray()))
    x = np.random.default_rng(13).standard_normal(L.n)

    def run(order):
        y = np.zeros(L.n)
        for t in order:
            rows, cols, A, X = work[int(items[t])]
            y[rows] += X @ (x[rows] - A @ y[cols])
        return y

    ref = run(range(len(items)))
    assert np.abs(ref).max() > 0
    for seed in range(5):
        rng = np.random.default_rng(seed)
        pred = pred0.copy()
        ready = np.flatnonzero(pred == 0).tolist()
        order = []
        while ready:
            t = ready.pop(int(rng.integers(len(ready))))
            order.append(t)
            for u in succ[sp[t]:sp[t + 1]]:
                pred[u] -= 1
                if pred[u] == 0:
                    ready.append(int(u))
        assert sorted(order) == list(range(len(items)))
        assert order != list(range(len(items)))
        assert np.array_equal(run(order), ref), seed


# ---- the refusals ----------------------------------------------------------------------------------------------------------------
def _refused(fn, *args):
    from alfi_amd._hostlib import PlanError
    with pytest.raises(PlanError) as e:
        fn(*args)
    assert e.value.code == E_ARG
    return str(e.value)


def _star(L):
    """one full 153-dof star of case b as a patch set of its own, and its hub node's position"""
    p = int(np.flatnonzero(np.diff(L.patch_ptr) == 153)[0])
    dofs = np.asarray(L.patch_dofs[L.patch_ptr[p]:L.patch_ptr[p + 1]])
    nodes = dofs[::L.bs] // L.bs
    hub = [i for i, v in enumerate(nodes) if np.isin(nodes, L.A.colidx[L.A.rowptr[v]:L.A.rowptr[v + 1]]).all()]
    assert len(hub) == 1
    return dofs, hub[0]


def test_refusals_of_the_condensed_plan():
    from alfi_amd import _hostlib
    La, _, _ = case("a")
    Lb, gb, _ = case("b")
    cond = _hostlib.plan_condensed
    bad = np.arange(len(La.patch_dofs), dtype=np.int32) // La.bs               # every node its own group: neighbours are coupled
    assert _refused(cond, La.bs, La.A.rowptr, La.A.colidx, La.patch_ptr, La.patch_dofs, bad) == (
        "patch 0: groups 0 and another one are coupled by an operator entry "
        "(a group may touch the rest of the patch only through unlabelled dofs)")
    dofs, hub = _star(Lb)
    pp = np.array([0, 153])
    args = (Lb.bs, Lb.A.rowptr, Lb.A.colidx)
    g = np.full(153, -1, dtype=np.int32)
    others = [i for i in range(51) if i != hub][:22]                           # 22 nodes: 66 entries in one group
    g.reshape(51, 3)[others] = 0
    msg = _refused(cond, *args, pp, dofs, g)
    assert msg.startswith("patch 0: group 0 holds 66 entries coupled to ") and msg.endswith(
        " skeleton entries; the condensed factors handle at most 64 of each")
    g[:] = -1
    g.reshape(51, 3)[hub] = 7                                                  # the hub alone: coupled to the 50 other nodes
    assert _refused(cond, *args, pp, dofs, g) == ("patch 0: group 7 holds 3 entries coupled to 150 skeleton entries; the "
                                                  "condensed factors handle at most 64 of each")
    g[:] = -1
    g[0] = 0                                                                   # a label on one component of a node
    assert _refused(cond, *args, pp, dofs, g) == "patch 0: entries of a node must be adjacent and carry one group label"
    g[:] = -1
    assert _refused(cond, *args, pp, dofs, g) == "no group label >= 0: nothing to condense"
    # patches of partial nodes: a dof short, and 150 entries that start inside a node
    assert _refused(cond, *args, np.array([0, 152]), dofs[1:], g[1:]) == "patch 0: condensed factors need patches of whole nodes"
    assert _refused(cond, *args, np.array([0, 150]), dofs[1:151], g[1:151]) == (
        "patch 0: entries of a node must be adjacent and carry one group label")


def test_refusals_of_the_sweep_schedule():
    from alfi_amd import _hostlib
    L, _, iterset = case("b")
    dofs, _ = _star(L)
    args = (L.bs, L.A.rowptr, L.A.colidx)
    it = iterset.copy()
    it[3] = len(L.patch_ptr) - 1
    assert _refused(_hostlib.plan_sweep, *args, L.patch_ptr, L.patch_dofs, it, True) == "iteration set entry out of range"
    it[3] = -1
    assert _refused(_hostlib.plan_sweep, *args, L.patch_ptr, L.patch_dofs, it, True) == "iteration set entry out of range"
    assert _refused(_hostlib.plan_sweep, *args, np.array([0, 153, 305]), np.concatenate([dofs, dofs[1:]]), [0, 1], True) == (
        "patch 1: multiplicative sweeps need patches of whole nodes")
    assert _refused(_hostlib.plan_sweep, *args, np.array([0, 150]), dofs[1:151], [0], True) == (
        "patch 0 does not consist of whole nodes")


def test_refusals_of_the_patch_layout():
    from alfi_amd import _hostlib
    lay = _hostlib.plan_patch_layout
    assert _refused(lay, 10, [0, 3, 6], [0, 1, 2, 4, 3, 5]) == "patch 1: dofs must be strictly ascending"
    assert _refused(lay, 10, [0, 3, 6], [0, 1, 2, 3, 3, 5]) == "patch 1: dofs must be strictly ascending"
    assert _refused(lay, 5, [0, 3, 6], [0, 1, 2, 3, 4, 5]) == "patch 1: dof 5 out of range"
    assert _refused(lay, 5, [0, 2], [-1, 2]) == "patch 0: dof -1 out of range"
    assert _refused(lay, 5000, [0, 4097], np.arange(4097)) == "patch 0 has 4097 dofs; supported range is 1..4096"
    assert _refused(lay, 10, [0, 2, 2], [0, 1]) == "patch 1 has 0 dofs; supported range is 1..4096"
    ok = lay(5000, [0, 4096], np.arange(4096))
    assert ok["max_np"] == 4096 and ok["sum_n2"] == 4096 * 4096
