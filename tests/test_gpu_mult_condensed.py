"""Multiplicative patch sweeps that read condensed patch factors (alfi_patches_set_multiplicative_condensed,
hip.Level.set_multiplicative(..., condensed=True), the option key patch_pc_patch_condensed_sweeps) against the oracle's
sequential sweep and against the dense sweep of a second level on the same patches and order.  -m gpu.

Levels, the smallest on which each path of the sweep can go wrong (all at Re = 100):
  a  ldc3d [P2+FB]^3, four cubes per side, finest level: 125 vertex stars of up to 153 dofs; the groups the level finds itself
     (find_patch_groups) handed back as the caller's.  Patches of at most 64 nodes, many patches per wavefront.
  b  2-D Scott-Vogelius [P2]^2 (build_sv_hierarchy, baseN 2, one refinement), macro_cell_groups: small macro stars.
  c  3-D Scott-Vogelius [P3]^3, ThreeDimLidDrivenCavityProblem(1), one refinement, macro_cell_groups: 27 macro stars of up to
     1599 dofs -- patches above 64 nodes, few per wavefront, several group chunks and sigma chunks each.
Orders: the problem's sort_order, a seeded random permutation, three patches with one of them twice; symmetrised and not.

Bounds: 1e-7 of the largest entry against the oracle and against the dense sweep (the bound tests/test_frontend.py uses for the
dense sweeps against the same oracle); the additive operator differs by more than 1e-3; full cycles 1e-5 (the same file)."""
import copy
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-7
CYCLE_TOL = 1e-5
CASES = ["a", "b", "c"]
ORDERS = ["sorted", "random", "short"]


def relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _problem(name):
    from alfi_amd.problem import ThreeDimLidDrivenCavityProblem, TwoDimLidDrivenCavityProblem
    return {"a": lambda: ThreeDimLidDrivenCavityProblem(2), "b": lambda: TwoDimLidDrivenCavityProblem(2),
            "c": lambda: ThreeDimLidDrivenCavityProblem(1)}[name]()


@functools.lru_cache(maxsize=None)
def hierarchy(name, Re):
    from alfi_amd.problem import build_hierarchy
    from alfi_amd.sv import build_sv_hierarchy
    if name == "a":
        return build_hierarchy(_problem(name), 1, 2, Re=Re)
    return build_sv_hierarchy(_problem(name), 1, 2 if name == "b" else 3, Re=Re)


@functools.lru_cache(maxsize=None)
def host_case(name):
    """(finest host level at Re = 100, its group labels, {order name: iteration set})"""
    from alfi_amd import _hostlib
    from alfi_amd.relaxation import Options, OrderedRelaxation
    L = hierarchy(name, 100.0)[0][-1]
    if name == "a":       # the rule of alfi_patches_find_groups on the host (tests/test_gpu_star_condense.py pins the two equal)
        groups = _hostlib.find_groups(L.bs, L.A.rowptr, L.A.colidx, L.patch_ptr, L.patch_dofs)
    else:
        groups = np.asarray(L.patch_groups, dtype=np.int32)
    npatch = len(L.patch_ptr) - 1
    orl = OrderedRelaxation()
    orl.name = "Star"
    orl.opts = Options("", {"pc_patch_construction_Star_sort_order": _problem(name).relaxation_direction()})
    mid = npatch // 2
    orders = {"sorted": np.asarray(orl.iteration_order(L.V.mesh.coords[L.patch_seeds]), dtype=np.int64),
              "random": np.random.default_rng(11).permutation(npatch).astype(np.int64),
              "short": np.array([mid, 0, npatch - 1, mid], dtype=np.int64)}
    assert sorted(orders["sorted"].tolist()) == list(range(npatch))
    return L, groups, orders


@functools.lru_cache(maxsize=None)
def oracle_smoother(name, Re):
    """the oracle's patch inverses of the case's operator at Re, computed once; ``sweep`` copies the handle, never the inverses"""
    from oracle import alfi_oracle as O
    L = host_case(name)[0]
    A = hierarchy(name, Re)[0][-1].A
    return O.PatchSmoother(A.to_scipy().tocsr(), L.patch_ptr, L.patch_dofs, L.bc_dofs)


def oracle_sweep(name, Re, iterset, symmetrise, x):
    sm = copy.copy(oracle_smoother(name, Re))
    sm.local_type, sm.iterset, sm.symmetrise = "multiplicative", np.asarray(iterset), symmetrise
    return sm.apply(x)


@functools.lru_cache(maxsize=None)
def rhs(name):
    return np.random.default_rng(3).standard_normal(host_case(name)[0].n)       # Dirichlet entries non-zero on purpose


@pytest.fixture(scope="module")
def ctx():
    from alfi_amd import hip
    c = hip.Context(0)
    yield c
    c.close()


def _level(ctx, name, groups=True):
    from alfi_amd import hip
    L, g, _ = host_case(name)
    dl = hip.Level(ctx, L.A, L.bc_dofs)
    dl.set_patches(L.patch_ptr, L.patch_dofs)
    dl.set_patch_groups(g if groups else None)
    dl.factor()
    assert dl.condensed() == (1 if groups else 0)
    return dl


@pytest.fixture(scope="module")
def levels(ctx):
    """per case one level with the caller's groups and one with dense inverses, made at first use and shared"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = (_level(ctx, name, True), _level(ctx, name, False))
        return made[name]
    yield get
    for pair in made.values():
        for dl in pair:
            dl.close()


def _apply(ctx, dl, x):
    dx, dy = ctx.vec(x), ctx.vec(len(x))
    dl.patch_apply(dx, dy)
    return dy.get()


def test_the_level_shapes_are_the_ones_the_cases_name():
    sizes = {n: np.diff(host_case(n)[0].patch_ptr) for n in CASES}
    assert sizes["a"].max() == 153 and len(sizes["a"]) == 125
    assert sizes["b"].max() <= 160 and sizes["b"].max() // 2 <= 64
    assert sizes["c"].max() // 3 > 64 and len(sizes["c"]) == 27


@pytest.mark.parametrize("symmetrise", [True, False], ids=["sym", "fwd"])
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", CASES)
def test_condensed_sweep_against_the_oracle_and_the_dense_sweep(ctx, levels, name, order, symmetrise):
    L, _, orders = host_case(name)
    it, x = orders[order], rhs(name)
    cl, dl = levels(name)
    bytes_before = cl.factor_bytes()
    nw = cl.set_multiplicative(it, symmetrise, condensed=True)
    assert cl.condensed() == 1 and cl.factor_bytes() == bytes_before          # the factors stay, and stay condensed
    assert dl.set_multiplicative(it, symmetrise) == nw and dl.condensed() == 0
    assert dl.factor_bytes() > bytes_before
    y = _apply(ctx, cl, x)
    assert np.array_equal(_apply(ctx, cl, x), y)                               # two applies, identical bits
    yd = _apply(ctx, dl, x)
    ref = oracle_sweep(name, 100.0, it, symmetrise, x)
    add = copy.copy(oracle_smoother(name, 100.0)).apply(x)
    print("%s %s %s: %d wavefronts; condensed against the oracle %.3e, against the dense sweep %.3e, dense against the oracle "
          "%.3e; additive against the sweep %.3e" % (name, order, "sym" if symmetrise else "fwd", nw, relerr(y, ref), relerr(y, yd),
                                                     relerr(yd, ref), relerr(add, ref)))
    assert relerr(y, ref) < TOL
    assert relerr(y, yd) < TOL
    assert relerr(add, y) > 1e-3                                               # it is not the additive apply
    assert np.array_equal(y[L.bc_dofs], x[L.bc_dofs])                          # Dirichlet entries copied exactly


@pytest.mark.parametrize("name", CASES)
def test_the_list_form_of_the_condensed_launches_has_the_bits_of_the_range_form(ctx, levels, name):
    """One visit of one patch from y = 0: the residual on its rows is x there, so the sweep leaves that patch's staged result --
    formed by the list kernels -- on its dofs.  The additive apply of a level that holds this patch alone forms the same result
    through the range kernels (fewer than 1024 patches: the chunked form), and adds it to zero."""
    from alfi_amd import hip
    L, g, _ = host_case(name)
    x = rhs(name)
    cl = levels(name)[0]
    sizes = np.diff(L.patch_ptr)
    # (patches with a group AND a skeleton: a level of its own needs both -- one patch without skeleton leaves the factorisation
    # of the Schur complements nothing to launch)
    grouped = [p for p in range(len(sizes)) if len(set((g[L.patch_ptr[p]:L.patch_ptr[p + 1]] >= 0).tolist())) == 2]
    for p in (max(grouped, key=lambda q: sizes[q]), min(grouped, key=lambda q: sizes[q])):      # the largest and the smallest
        a, b = L.patch_ptr[p], L.patch_ptr[p + 1]
        dofs = L.patch_dofs[a:b]
        cl.set_multiplicative([p], False, condensed=True)
        y = _apply(ctx, cl, x)
        one = hip.Level(ctx, L.A, L.bc_dofs)
        one.set_patches(np.array([0, b - a]), dofs)
        one.set_patch_groups(g[a:b])
        one.factor()
        assert one.condensed() == 1
        ya = _apply(ctx, one, x)
        one.close()
        assert np.abs(ya[dofs]).max() > 0.0 and np.array_equal(y[dofs], ya[dofs])
        rest = np.setdiff1d(np.arange(L.n), np.concatenate([dofs, L.bc_dofs]))
        assert not y[rest].any()


@pytest.mark.parametrize("name", CASES)
def test_new_operator_values_are_refactored_into_the_condensed_factors(ctx, name):
    L, _, orders = host_case(name)
    it, x = orders["sorted"], rhs(name)
    cl = _level(ctx, name, True)
    cl.set_multiplicative(it, True, condensed=True)
    y100 = _apply(ctx, cl, x)
    cl.update_values(hierarchy(name, 10.0)[0][-1].A.vals)
    cl.factor()
    assert cl.condensed() == 1
    y = _apply(ctx, cl, x)
    ref = oracle_sweep(name, 10.0, it, True, x)
    print("%s: Re 10 against the oracle %.3e; against the Re 100 sweep %.3e" % (name, relerr(y, ref), relerr(y, y100)))
    assert relerr(y, ref) < TOL
    assert relerr(y100, ref) > 1e-3                                            # the operators do differ
    cl.close()


@pytest.mark.parametrize("name", CASES)
def test_back_to_additive_keeps_the_bits_of_the_additive_apply(ctx, name):
    _, _, orders = host_case(name)
    x = rhs(name)
    cl = _level(ctx, name, True)
    before = _apply(ctx, cl, x)
    for how in (dict(condensed=True), dict()):                                 # nit == 0 through either call
        assert cl.set_multiplicative(orders["random"], True, condensed=True) > 0
        assert relerr(_apply(ctx, cl, x), before) > 1e-3
        assert cl.set_multiplicative(None, False, **how) == 0
        assert cl.condensed() == 1
        assert np.array_equal(_apply(ctx, cl, x), before)                      # the staging buffer is shared with the sweeps
    cl.close()


def test_a_level_without_groups_takes_the_dense_call():
    """without the caller's groups the new call IS alfi_patches_set_multiplicative -- also on a level that condensed itself"""
    from alfi_amd import hip
    L, _, orders = host_case("a")
    it, x = orders["sorted"], rhs("a")
    c = hip.Context(0)
    c.set_condense_min_bytes(0)                                                # every level condenses where it finds groups
    out = []
    for condensed in (True, False):
        dl = hip.Level(c, L.A, L.bc_dofs)
        dl.set_patches(L.patch_ptr, L.patch_dofs)
        dl.factor()
        assert dl.condensed() == 2
        small = dl.factor_bytes()
        dl.set_multiplicative(it, True, condensed=condensed)
        assert dl.condensed() == 0 and dl.factor_bytes() > small
        out.append(_apply(c, dl, x))
        dl.close()
    assert np.array_equal(out[0], out[1])
    c.close()


def test_refusals(ctx):
    from alfi_amd import hip
    L, g, orders = host_case("a")
    it = orders["sorted"]
    # partition of unity, on a level with the caller's groups
    cl = _level(ctx, "a", True)
    cl.set_partition_of_unity(True)
    with pytest.raises(hip.AlfiHipError, match="partition of unity") as e:
        cl.set_multiplicative(it, True, condensed=True)
    assert e.value.code == hip.E_STATE
    cl.set_partition_of_unity(False)
    # an iteration set out of range
    with pytest.raises(hip.AlfiHipError, match="out of range") as e:
        cl.set_multiplicative([0, len(L.patch_ptr)], True, condensed=True)
    assert e.value.code == hip.E_ARG
    # the old call still refuses the caller's groups; new groups on a level that sweeps stay refused
    with pytest.raises(hip.AlfiHipError, match="dense patch inverses") as e:
        cl.set_multiplicative(it, True)
    assert e.value.code == hip.E_STATE
    cl.set_multiplicative(it, True, condensed=True)
    with pytest.raises(hip.AlfiHipError, match="multiplicative sweeps"):
        cl.set_patch_groups(g)
    cl.close()
    # FP32 storage (a level with the caller's groups cannot ask for it: the request is refused there)
    fl = _level(ctx, "a", False)
    fl.set_patch_storage("f32")
    with pytest.raises(hip.AlfiHipError, match="FP32 patch storage") as e:
        fl.set_multiplicative(it, True, condensed=True)
    assert e.value.code == hip.E_STATE
    fl.close()
    # a partitioned level (one rank owning every node, marked distributed) with the caller's groups
    pl = hip.Level(ctx, L.A, L.bc_dofs)
    pl.set_partition(L.A.nbrows, True, np.zeros(0, dtype=np.int32), None, None, 0)
    pl.set_patches(L.patch_ptr, L.patch_dofs)
    pl.set_patch_groups(g)
    with pytest.raises(hip.AlfiHipError, match="partitioned") as e:
        pl.set_multiplicative(it, True, condensed=True)
    assert e.value.code == hip.E_ARG
    pl.close()


def test_groups_withdrawn_from_a_sweeping_level_give_the_dense_sweep(ctx, levels):
    """set_patch_groups(None) on a level in the new mode drops the condensed storage; after the next factorisation the sweeps read
    dense inverses and have the bits of a level that never held groups"""
    _, _, orders = host_case("b")
    it, x = orders["sorted"], rhs("b")
    cl = _level(ctx, "b", True)
    cl.set_multiplicative(it, True, condensed=True)
    small = cl.factor_bytes()
    cl.set_patch_groups(None)
    cl.factor()
    assert cl.condensed() == 0 and cl.factor_bytes() > small
    dl = levels("b")[1]
    dl.set_multiplicative(it, True)
    assert np.array_equal(_apply(ctx, cl, x), _apply(ctx, dl, x))
    cl.close()


def test_built_in_vertex_stars_get_the_groups_the_level_finds(ctx):
    """case a through HipPatchPC: the built-in star construction with local_type multiplicative and the key -- the level's own
    find_patch_groups() handed back as the caller's groups; without the key the level keeps dense inverses"""
    import alfi_amd
    L, g, _ = host_case("a")
    x = rhs("a")
    out = {}
    for key in (True, False):
        opts = alfi_amd.mg_levels_solver(3)
        assert opts["patch_pc_patch_construct_type"] == "star"
        opts.update({"patch_pc_patch_local_type": "multiplicative", "patch_pc_patch_symmetrise_sweep": True})
        if key:
            opts["patch_pc_patch_condensed_sweeps"] = True
        pc = alfi_amd.PC(ctx, L, options=opts)
        obj = alfi_amd.HipPatchPC()
        obj.initialize(pc)
        assert obj.condensed == key and obj.level.condensed() == (1 if key else 0) and obj.wavefronts > 1
        assert np.array_equal(obj.patch_ptr, L.patch_ptr) and np.array_equal(obj.patch_dofs, L.patch_dofs)
        y = np.zeros(L.n)
        obj.apply(pc, x, y)
        out[key] = (y, obj.level.factor_bytes(), np.asarray(obj.iterset))
        obj.level.close()
    ref = oracle_sweep("a", 100.0, out[True][2], True, x)
    print("built-in stars: condensed against the oracle %.3e, dense %.3e; bytes %d / %d"
          % (relerr(out[True][0], ref), relerr(out[False][0], ref), out[True][1], out[False][1]))
    assert relerr(out[True][0], ref) < TOL
    assert relerr(out[True][0], out[False][0]) < TOL
    assert out[True][1] < out[False][1]


def test_full_cycles_through_the_option_key(ctx):
    """case b through HipMG: patch_pc_patch_condensed_sweeps with two smoothing steps against the oracle's full cycle"""
    import alfi_amd
    from oracle import alfi_oracle as O
    lv, tr = hierarchy("b", 100.0)
    L = lv[-1]
    prob = _problem("b")
    plain = alfi_amd.mg_levels_solver(2, patch="macro", patch_composition="multiplicative", smoothing=2,
                                      relaxation_direction=prob.relaxation_direction())
    opts = alfi_amd.mg_levels_solver(2, patch="macro", patch_composition="multiplicative", smoothing=2,
                                     relaxation_direction=prob.relaxation_direction(), condensed_sweeps=True)
    assert "patch_pc_patch_condensed_sweeps" not in plain and opts["patch_pc_patch_condensed_sweeps"] is True
    b = np.random.default_rng(4).standard_normal(L.n)
    b[L.bc_dofs] = 0.0
    out = {}
    for key, o in (("condensed", opts), ("dense", plain)):
        mg = alfi_amd.HipMG(ctx, lv, tr, alfi_amd.fieldsplit_0_mg(o))
        assert [d.condensed() for d in mg.mg.levels[1:]] == [1 if key == "condensed" else 0] * (len(lv) - 1)
        assert all(p.wavefronts >= 1 for p in mg.pc_objs[1:])
        y = np.zeros(L.n)
        mg.apply(b, y)
        out[key] = y
        itersets = [None] + [p.iterset for p in mg.pc_objs[1:]]
        patches = [(p.patch_ptr, p.patch_dofs) for p in mg.pc_objs[1:]]
        mg.mg.close()
    olv = [copy.copy(Lv) for Lv in lv]
    for Lv, (pp, pd) in zip(olv[1:], patches):
        Lv.patch_ptr, Lv.patch_dofs = pp, pd
    ref = O.build_oracle_mg(olv, tr, 2, local_type="multiplicative", itersets=itersets, symmetrise=True).fcycle(b)
    print("full cycle against the oracle: condensed %.3e, dense %.3e" % (relerr(out["condensed"], ref), relerr(out["dense"], ref)))
    assert relerr(out["condensed"], ref) < CYCLE_TOL
