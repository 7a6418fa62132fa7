"""CPU checks of the single-precision storage of dense patch inverses (csrc/patch_plan.h: f32_inv_index, plan_f32_offsets)
through libalfi_host.so: the index map the conversion kernel writes with and alfi_patch_get_inverse reads with, and the
offsets the apply kernel's vector loads rely on."""
import numpy as np
import pytest

from alfi_amd import _hostlib


@pytest.mark.parametrize("n", range(1, 161))
def test_index_map_is_a_bijection_into_the_padded_rows(n):
    lay = _hostlib.plan_f32_layout(np.array([0, n]))
    V = lay["rows_per_load"]
    ld, floats, idx = _hostlib.f32_index(n)
    assert ld == (n + V - 1) // V * V and idx.shape == (ld, n)
    # every stored row, pad rows included, has a place of its own in [0, ld * n): nothing beyond, nothing twice
    assert np.array_equal(np.sort(idx.ravel()), np.arange(ld * n))
    assert ld * n <= floats and floats % lay["align_floats"] == 0 and floats - ld * n < lay["align_floats"]
    # the n x n entries never land on a pad position, and the pad rows fill exactly the rest
    real, pad = idx[:n].ravel(), idx[n:].ravel()
    assert len(np.unique(real)) == n * n and len(np.intersect1d(real, pad)) == 0
    # a lane's V rows of a column are V consecutive floats on a V-float boundary: one aligned vector load
    for r in range(0, ld, V):
        assert np.all(idx[r] % V == 0)
        for k in range(1, V):
            assert np.array_equal(idx[r + k], idx[r] + k)


def test_pieces_are_stored_column_by_column():
    # rows padded to V: as many 128-row pieces as fit, then the binary digits of the remainder, each [column][rows of the piece]
    # (153 rows with V = 4: 156 padded = 128 + 16 + 8 + 4)
    for n in (153, 111, 160, 33, 5):
        ld, _, idx = _hostlib.f32_index(n)
        V = _hostlib.plan_f32_layout(np.array([0, n]))["rows_per_load"]
        pieces = [128] * (ld // 128) + [b for b in (64, 32, 16, 8, 4, 2) if b >= V and (ld % 128) & b]
        assert sum(pieces) == ld and (n != 153 or V != 4 or pieces == [128, 16, 8, 4])
        row0 = 0
        for rows in pieces:
            r, c = np.meshgrid(np.arange(rows), np.arange(n), indexing="ij")
            assert np.array_equal(idx[row0:row0 + rows], row0 * n + c * rows + r)
            row0 += rows


def test_offsets_of_a_mixed_patch_set():
    rng = np.random.default_rng(3)
    sizes = np.concatenate([rng.integers(1, 161, 200), [1, 2, 3, 4, 5, 33, 127, 128, 129, 153, 159, 160]])
    pp = np.concatenate([[0], np.cumsum(sizes)])
    lay = _hostlib.plan_f32_layout(pp)
    ptr, V, align = lay["f32_ptr"], lay["rows_per_load"], lay["align_floats"]
    assert ptr[0] == 0 and len(ptr) == len(sizes) + 1 and ptr[-1] == lay["inv32_floats"]
    assert np.all(np.diff(ptr) > 0)
    # the apply's vector loads need 4 * V bytes; every patch starts on a 128-byte line
    assert align * 4 == 128 and align % V == 0 and np.all(ptr % align == 0)
    for n, a, b in zip(sizes, ptr[:-1], ptr[1:]):
        assert b - a == _hostlib.f32_index(int(n))[1]
    # half the FP64 layout's bytes, up to the padding of rows and lines
    f64 = _hostlib.plan_patch_layout(int(pp[-1]), pp, np.arange(pp[-1], dtype=np.int32))["inv_doubles"] * 8
    assert 4 * ptr[-1] < 0.55 * f64


def test_a_patch_beyond_the_kernel_is_refused():
    with pytest.raises(_hostlib.PlanError) as e:
        _hostlib.plan_f32_layout(np.array([0, 40, 201]))
    assert e.value.code == -2 and "161" in str(e.value)


def test_a_rank_knows_the_order_of_the_unpartitioned_patch():
    """dist.localize_level: ``patch_rank`` lists, per local patch entry, its place in the global patch (ascending global dofs) --
    the elimination order an FP32 level follows (alfi_patches_set_canonical_order) so that its float32 values do not depend on
    the partition."""
    from alfi_amd import dist as D
    from alfi_amd.problem import ThreeDimLidDrivenCavityProblem, build_hierarchy
    lv, tr = build_hierarchy(ThreeDimLidDrivenCavityProblem(2), 1, 1, Re=10.0)
    L = lv[-1]
    world = 3
    splits = D.choose_splits(lv, world, 1)
    permuted = 0
    for r in range(world):
        part = D.LevelPart(L.level, L.bs, splits[L.level], r, D.compute_ghosts(lv, tr, splits, L.level, r))
        LL = D.localize_level(L, part)
        l2g = (part.nodes[:, None] * L.bs + np.arange(L.bs)).ravel()
        assert len(LL.patch_rank) == len(LL.patch_dofs) and LL.patch_rank.dtype == np.int32
        for p, gp in enumerate(LL.patch_ids):
            a, b = LL.patch_ptr[p], LL.patch_ptr[p + 1]
            rank, gd = LL.patch_rank[a:b], l2g[LL.patch_dofs[a:b]]
            assert np.array_equal(np.sort(rank), np.arange(b - a))
            want = L.patch_dofs[L.patch_ptr[gp]:L.patch_ptr[gp + 1]]
            got = np.empty(b - a, dtype=np.int64)
            got[rank] = gd
            assert np.array_equal(got, want)
            permuted += int(not np.array_equal(rank, np.arange(b - a)))
    assert permuted > 0          # ghosts are numbered last: some patch's local order is not the global one


def _documented_layout(n, ld, min_rows):
    """(ld, n) offsets of the row-piece storage as patch_plan.h documents it: as many 128-row pieces as fit, then the binary
    digits of the remainder down to min_rows, a piece of R rows stored [column][R], the pieces one after the other"""
    pieces = [128] * (ld // 128) + [b for b in (64, 32, 16, 8, 4, 2) if b >= min_rows and (ld % 128) & b]
    assert sum(pieces) == ld
    idx = np.empty((ld, n), dtype=np.int64)
    row0 = 0
    for rows in pieces:
        r, c = np.meshgrid(np.arange(rows), np.arange(n), indexing="ij")
        idx[row0:row0 + rows] = row0 * n + c * rows + r
        row0 += rows
    return idx


@pytest.mark.parametrize("min_rows", [2, 4])
def test_the_unified_index_is_the_documented_layout_and_the_wrappers_are_it(min_rows):
    """piece_index (csrc/patch_plan.h), the one loop over the binary digits: a bijection onto [0, ld n) that equals the documented
    layout, for every n the FP64 / FP32 kernels of small patches see and well into the macro stars; patch_inv_index (min_rows 2)
    and f32_inv_index (min_rows 4) are it."""
    for n in range(1, 601):
        ld = (n + min_rows - 1) // min_rows * min_rows
        idx = _hostlib.piece_index_table(n, ld, min_rows)
        assert idx.min() == 0 and np.array_equal(np.bincount(idx.ravel(), minlength=ld * n), np.ones(ld * n, dtype=np.int64)), n
        assert np.array_equal(idx, _documented_layout(n, ld, min_rows)), n
        if min_rows == 2:
            assert np.array_equal(_hostlib.patch_index_table(n), idx), n
        else:
            wld, _, widx = _hostlib.f32_index_table(n)
            assert wld == ld and np.array_equal(widx, idx), n
