"""Adjoint solves on partitioned levels, the device-free part (-m "not gpu"): the ABI of the transposed operator refresh
(alfi_level_set_assembly_transposed), and the preconditions that make it exact on a rank's local level -- the localised
sparsity is structurally symmetric, and the contributor lists of block (i, j) and of its mirror (j, i) hold the same cells /
facets in the same order with the two local indices swapped.  With these a rank forms its rows of A^T from the lists it
already has, bitwise the forward values of the mirror blocks; a failure of the GPU tests is then the kernels', not the lists'."""
import functools
import os
import re

import numpy as np
import pytest

from alfi_amd import _hostlib
from alfi_amd.dist import FacetPart, assembly_cells, build_parts, choose_splits, localize
from alfi_amd.problem import TwoDimLidDrivenCavityProblem, build_hierarchy
from alfi_amd.sv import build_sv_hierarchy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "alfi_level_set_assembly_transposed"


def test_transposed_refresh_is_declared_exported_and_bound():
    """Fails without the feature: the header declares the switch, the library exports it, _lib binds it."""
    import ctypes
    from alfi_amd import _lib
    text = open(os.path.join(ROOT, "include", "alfi_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(\s*alfi_level\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)\s*;" % NAME, text)
    assert hasattr(_lib.load(), NAME)
    assert _lib.SIGNATURES[NAME] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int])
    from alfi_amd import hip
    assert callable(hip.Level.set_assembly_transposed)


@functools.lru_cache(maxsize=None)
def _hierarchy(case):
    if case == "pkp0":
        return build_hierarchy(TwoDimLidDrivenCavityProblem(4), 2, 2, Re=0.0)
    return build_sv_hierarchy(TwoDimLidDrivenCavityProblem(4), 2, 2, Re=0.0, facet_coupling=True)


@functools.lru_cache(maxsize=None)
def _rank_levels(case, world):
    """(global levels, [(rank, local level)]) for every rank and every level it owns rows of, every level partitioned."""
    levels, transfers = _hierarchy(case)
    splits = choose_splits(levels, world, min_dofs=1)
    out = []
    for rank in range(world):
        parts = build_parts(levels, transfers, splits, rank, exchange_lists=None)
        llev, _, _ = localize(levels, transfers, parts)
        out.extend((rank, LL) for LL in llev if LL.part.nb_own > 0)
    return levels, out


def _mirror(rowptr, colidx):
    """Index of block (j, i) for every block (i, j); the columns of a localised row are not sorted."""
    n = len(rowptr) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    key, mkey = rows * n + colidx, np.asarray(colidx, dtype=np.int64) * n + rows
    assert np.unique(key).size == key.size
    order = np.argsort(key)
    pos = np.searchsorted(key[order], mkey)
    assert (pos < key.size).all() and np.array_equal(key[order][np.minimum(pos, key.size - 1)], mkey), "sparsity not symmetric"
    return order[pos]


def _assert_mirrored_lists(ptr, item, code, base, mirror, swap_div):
    """Per block k: the list of mirror[k] has the same items in the same order, the pair code with its two indices swapped."""
    lens = np.diff(ptr)
    assert np.array_equal(lens, lens[mirror])
    # entries of mirror[k], laid out in the order of k's entries
    start = np.repeat(ptr[mirror], lens) + (np.arange(ptr[-1]) - np.repeat(ptr[:-1], lens))
    assert np.array_equal(item, item[start])
    hi, lo = code.astype(np.int64) // swap_div, code.astype(np.int64) % swap_div
    assert np.array_equal(lo * base + hi, code[start].astype(np.int64))


CASES = [pytest.param(c, w, id="%s-%dranks" % (c, w)) for c in ("pkp0", "sv-burman") for w in (2, 3)]


@pytest.mark.parametrize("case,world", CASES)
def test_local_sparsity_is_symmetric_and_cell_lists_mirror(case, world):
    levels, ranks = _rank_levels(case, world)
    seen, ghost_rows = set(), 0
    for rank, LL in ranks:
        L, part = levels[LL.level], LL.part
        rp, ci = np.asarray(LL.A.rowptr, dtype=np.int64), np.asarray(LL.A.colidx, dtype=np.int64)
        assert len(rp) - 1 == part.nb_loc and ci.max() < part.nb_loc
        mirror = _mirror(rp, ci)
        assert np.array_equal(mirror[mirror], np.arange(ci.size))
        if case == "pkp0":
            cells, cn, nodes = assembly_cells(L.V, part)
        else:
            cn = FacetPart(L.V, L.facets, part).cell_nodes
        nloc = cn.shape[1]
        cptr, ccell, cba = _hostlib.contributors(cn, part.nb_loc, rp, ci, nindex=int(cn.max()) + 1, partial=True)
        block_of = np.repeat(np.arange(ci.size), np.diff(cptr))
        same = block_of[1:] == block_of[:-1]
        assert np.all(np.diff(ccell.astype(np.int64))[same] > 0)          # cells ascending within every block's list
        _assert_mirrored_lists(cptr, ccell, cba, nloc, mirror, nloc)      # cba = b * nloc + a
        seen.add(rank)
        ghost_rows += part.nb_loc - part.nb_own
    assert seen == set(range(world)) and ghost_rows > 0


@pytest.mark.parametrize("world", [2, 3])
def test_facet_lists_mirror(world):
    levels, ranks = _rank_levels("sv-burman", world)
    pairs = 0
    for rank, LL in ranks:
        L, part = levels[LL.level], LL.part
        rp, ci = np.asarray(LL.A.rowptr, dtype=np.int64), np.asarray(LL.A.colidx, dtype=np.int64)
        mirror = _mirror(rp, ci)
        fp = FacetPart(L.V, L.facets, part)
        (bptr, bfac, bab), _ = fp.lists(LL.A)
        nu = int(fp.table.nu)
        _assert_mirrored_lists(np.asarray(bptr), np.asarray(bfac), np.asarray(bab), nu, mirror, nu)      # bab = a * nu + b
        pairs += int(bptr[-1])
    assert pairs > 0
