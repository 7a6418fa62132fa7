"""The work lists of multiplicative sweeps that read condensed patch factors (csrc/patch_plan.h: plan_sweep_condensed, what
alfi_patches_set_multiplicative_condensed uploads) through the export of libalfi_host.so, on the patch sets of
tests/patch_plan_cases.py and on one made for the edges: a patch without any interior group (it contributes no group chunk)
and an iteration set that visits a patch twice.  No GPU.

Per dependency wavefront w the lists are the concatenation, over the wavefront's patches in seq order, of the patch's group
chunks [gcptr[p], gcptr[p+1]), of its sigma chunks [chptr[p], chptr[p+1]) and of its block rows; the reverse pass of a symmetrised
sweep walks the same wavefronts backwards and has no table of its own."""
import numpy as np
import pytest

from alfi_amd import _hostlib
from tests.patch_plan_cases import case, plans


def _expected(L, sweep, cond):
    pp, pd, bs = np.asarray(L.patch_ptr), np.asarray(L.patch_dofs), L.bs
    gk, sk, nd, wk, wc, wn = [], [], [], [0], [0], [0]
    for w in range(len(sweep["wave_ptr"]) - 1):
        for p in sweep["seq"][sweep["wave_ptr"][w]:sweep["wave_ptr"][w + 1]]:
            gk += range(cond["gcptr"][p], cond["gcptr"][p + 1])
            sk += range(cond["chptr"][p], cond["chptr"][p + 1])
            nd += (pd[pp[p]:pp[p + 1]:bs] // bs).tolist()
        wk.append(len(gk))
        wc.append(len(sk))
        wn.append(len(nd))
    return {"gchunk": gk, "schunk": sk, "node": nd, "wk_ptr": wk, "wc_ptr": wc, "wn_ptr": wn}


def _check(L, iterset, sweep, cond):
    sc = _hostlib.plan_sweep_condensed(L.bs, L.patch_ptr, L.patch_dofs, sweep, cond)
    exp = _expected(L, sweep, cond)
    for k, v in exp.items():
        assert np.array_equal(sc[k], np.asarray(v, dtype=sc[k].dtype)), k
    assert sc["gchunk"].dtype == np.int32 and sc["wk_ptr"].dtype == np.int64
    # every chunk of every iterated patch once per visit, chunks of the other patches never
    npatch = len(L.patch_ptr) - 1
    visits = np.bincount(np.asarray(iterset), minlength=npatch)
    ngc, nch = int(cond["gcptr"][-1]), int(cond["chptr"][-1])
    gc_patch = np.repeat(np.arange(npatch), np.diff(cond["gcptr"]))
    ch_patch = np.repeat(np.arange(npatch), np.diff(cond["chptr"]))
    assert np.array_equal(np.bincount(sc["gchunk"], minlength=ngc), visits[gc_patch])
    assert np.array_equal(np.bincount(sc["schunk"], minlength=nch), visits[ch_patch])
    assert np.array_equal(ch_patch, cond["ch_patch"][:nch])
    # a wavefront's patches share no block row
    for w in range(len(sc["wn_ptr"]) - 1):
        rows = sc["node"][sc["wn_ptr"][w]:sc["wn_ptr"][w + 1]]
        assert len(np.unique(rows)) == len(rows)
    return sc


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_wavefront_lists_on_the_planner_cases(name):
    L, groups, iterset = case(name)
    pl = plans(name)
    sc = _check(L, iterset, pl["sweep"], pl["cond"])
    assert len(sc["wk_ptr"]) == len(pl["sweep"]["wave_ptr"])
    if name == "c":        # macro stars of several group chunks and several sigma chunks each
        assert np.diff(pl["cond"]["gcptr"]).max() > 1 and np.diff(pl["cond"]["chptr"]).max() > 1
    if name == "a":        # "0+:1-|1+:0-": two sweeps, every patch twice
        assert np.bincount(iterset).min() == 2


def test_a_patch_without_interior_group_and_a_patch_visited_twice():
    L, groups, _ = case("a")
    pp = np.asarray(L.patch_ptr)
    npatch = len(pp) - 1
    g = np.array(groups, dtype=np.int32)
    bare = int(np.argmax(np.diff(pp)))                  # the largest star loses its labels: all skeleton
    assert (g[pp[bare]:pp[bare + 1]] >= 0).any()
    g[pp[bare]:pp[bare + 1]] = -1
    cond = _hostlib.plan_condensed(L.bs, L.A.rowptr, L.A.colidx, L.patch_ptr, L.patch_dofs, g)
    assert cond["gcptr"][bare] == cond["gcptr"][bare + 1] and cond["chptr"][bare + 1] > cond["chptr"][bare]
    other = (bare + 1) % npatch
    iterset = np.array([other, bare, (bare + 2) % npatch, bare], dtype=np.int64)      # three patches, one twice
    for sym in (True, False):
        sweep = _hostlib.plan_sweep(L.bs, L.A.rowptr, L.A.colidx, L.patch_ptr, L.patch_dofs, iterset, sym)
        sc = _check(L, iterset, sweep, cond)
        assert len(sc["schunk"]) == sum(cond["chptr"][p + 1] - cond["chptr"][p] for p in iterset)
        # the two visits of the bare patch lie in different wavefronts and add no group chunk to either
        waves = [w for w in range(len(sweep["wave_ptr"]) - 1)
                 if bare in sweep["seq"][sweep["wave_ptr"][w]:sweep["wave_ptr"][w + 1]]]
        assert len(waves) == 2
        for w in waves:
            seq = sweep["seq"][sweep["wave_ptr"][w]:sweep["wave_ptr"][w + 1]]
            assert sc["wk_ptr"][w + 1] - sc["wk_ptr"][w] == sum(cond["gcptr"][p + 1] - cond["gcptr"][p] for p in seq if p != bare)


def test_a_sequence_entry_out_of_range_is_refused():
    L, groups, iterset = case("a")
    pl = plans("a")
    bad = dict(pl["sweep"])
    bad["seq"] = pl["sweep"]["seq"].copy()
    bad["seq"][0] = len(L.patch_ptr) - 1
    with pytest.raises(_hostlib.PlanError, match="out of range") as e:
        _hostlib.plan_sweep_condensed(L.bs, L.patch_ptr, L.patch_dofs, bad, pl["cond"])
    assert e.value.code == -2
