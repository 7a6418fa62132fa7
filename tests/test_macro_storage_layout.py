"""CPU checks of the single-precision storage of dense MACRO-STAR inverses (alfi_patches_set_macro_storage) through
libalfi_host.so: the layout of csrc/patch_plan.h (f32_inv_index, plan_f32_offsets) beyond 160 dofs, where big_apply_kernel<float, NT>
reads it -- the assertions tests/test_patch_storage_layout.py makes up to 160."""
import numpy as np
import pytest

from alfi_amd import _hostlib

SIZES = (161, 162, 163, 164, 255, 256, 257, 385, 513, 1599, 1600, 4095, 4096)


@pytest.mark.parametrize("n", SIZES)
def test_index_map_is_a_bijection_into_the_padded_rows(n):
    lay = _hostlib.plan_macro_f32_layout(np.array([0, n]))
    V = lay["rows_per_load"]
    ld, floats, idx = _hostlib.f32_index_table(n)
    assert ld == (n + V - 1) // V * V and idx.shape == (ld, n)
    # every stored row, pad rows included, has a place of its own in [0, ld * n): nothing beyond, nothing twice
    hits = np.bincount(idx.ravel(), minlength=ld * n)
    assert idx.min() == 0 and len(hits) == ld * n and np.all(hits == 1)
    assert ld * n <= floats and floats % lay["align_floats"] == 0 and floats - ld * n < lay["align_floats"]
    assert floats == lay["inv32_floats"]
    # the pad rows fill exactly what the n x n entries leave (the map is a bijection: the two sets are disjoint)
    assert idx[:n].size == n * n and idx[n:].size == (ld - n) * n
    # a lane's V rows of a column are V consecutive floats on a V-float boundary: one aligned vector load
    assert np.all(idx[0::V] % V == 0)
    for k in range(1, V):
        assert np.array_equal(idx[k::V], idx[0::V] + k)
    # the bulk export is the entry-wise one
    L = _hostlib.lib()
    rng = np.random.default_rng(n)
    for r, c in zip(rng.integers(0, ld, 50), rng.integers(0, n, 50)):
        assert L.alfi_host_f32_index(int(r), int(c), n) == idx[r, c]


@pytest.mark.parametrize("n", SIZES)
def test_pieces_are_stored_column_by_column(n):
    # rows padded to V: as many 128-row pieces as fit, then the binary digits of the remainder down to V, each
    # [column][rows of the piece] (1599 rows: 1600 padded = 12 x 128 + 64)
    ld, _, idx = _hostlib.f32_index_table(n)
    V = _hostlib.plan_macro_f32_layout(np.array([0, n]))["rows_per_load"]
    pieces = [128] * (ld // 128) + [b for b in (64, 32, 16, 8, 4, 2) if b >= V and (ld % 128) & b]
    assert sum(pieces) == ld and (n != 1599 or V != 4 or pieces == [128] * 12 + [64])
    row0 = 0
    for rows in pieces:
        r, c = np.meshgrid(np.arange(rows), np.arange(n), indexing="ij")
        assert np.array_equal(idx[row0:row0 + rows], row0 * n + c * rows + r)
        row0 += rows


def test_offsets_of_a_mixed_patch_set():
    rng = np.random.default_rng(5)
    sizes = np.concatenate([rng.integers(1, 161, 40), rng.integers(161, 4097, 40),
                            [159, 160, 161, 162, 163, 164, 1599, 4095, 4096, 33, 150]])
    rng.shuffle(sizes)
    pp = np.concatenate([[0], np.cumsum(sizes)])
    lay = _hostlib.plan_macro_f32_layout(pp)
    ptr, V, align = lay["f32_ptr"], lay["rows_per_load"], lay["align_floats"]
    assert ptr[0] == 0 and len(ptr) == len(sizes) + 1 and ptr[-1] == lay["inv32_floats"]
    assert np.all(np.diff(ptr) > 0)
    # the apply's vector loads need 4 * V bytes; every patch starts on a 128-byte line
    assert align * 4 == 128 and align % V == 0 and np.all(ptr % align == 0)
    L = _hostlib.lib()
    for n, a, b in zip(sizes, ptr[:-1], ptr[1:]):
        ld = (int(n) + V - 1) // V * V
        assert b - a == L.alfi_host_f32_patch_floats(int(n)) and 0 <= b - a - ld * int(n) < align
    # where both layouts exist they agree
    small = np.concatenate([[0], np.cumsum(sizes[sizes <= 160])])
    assert np.array_equal(_hostlib.plan_macro_f32_layout(small)["f32_ptr"], _hostlib.plan_f32_layout(small)["f32_ptr"])
    # half the FP64 layout's bytes, up to the padding of rows and lines
    f64 = _hostlib.plan_patch_layout(int(pp[-1]), pp, np.arange(pp[-1], dtype=np.int32))["inv_doubles"] * 8
    assert 4 * ptr[-1] < 0.55 * f64


def test_a_patch_beyond_the_big_patch_kernels_is_refused():
    with pytest.raises(_hostlib.PlanError) as e:
        _hostlib.plan_macro_f32_layout(np.array([0, 40, 4137]))
    assert e.value.code == -2 and "4097" in str(e.value)


def test_both_layout_entry_points_return_what_they_returned():
    # one implementation behind the two: the same offsets and scalars as before (entry by entry from the per-patch export), each
    # with its own limit and its own wording
    sizes = np.array([33, 160, 1, 159, 64, 150])
    pp = np.concatenate([[0], np.cumsum(sizes)])
    L = _hostlib.lib()
    floats = [L.alfi_host_f32_patch_floats(int(n)) for n in sizes]
    for plan in (_hostlib.plan_f32_layout, _hostlib.plan_macro_f32_layout):
        lay = plan(pp)
        assert sorted(lay) == ["align_floats", "f32_ptr", "inv32_floats", "rows_per_load"]
        assert np.array_equal(lay["f32_ptr"], np.concatenate([[0], np.cumsum(floats)])) and lay["inv32_floats"] == sum(floats)
        assert lay["rows_per_load"] == 4 and lay["align_floats"] == 32
    with pytest.raises(_hostlib.PlanError) as e:
        _hostlib.plan_f32_layout(np.array([0, 40, 201]))
    assert e.value.code == -2 and str(e.value) == "patch 1 has 161 dofs; FP32 storage holds patches of 1..160"
    assert len(_hostlib.plan_f32_layout(np.array([0, 40, 200]))["f32_ptr"]) == 3
    with pytest.raises(_hostlib.PlanError) as e:
        _hostlib.plan_macro_f32_layout(np.array([0, 40, 4137]))
    assert e.value.code == -2 and str(e.value) == "patch 1 has 4097 dofs; FP32 macro-star storage holds patches of 1..4096"
    assert len(_hostlib.plan_macro_f32_layout(np.array([0, 40, 4136]))["f32_ptr"]) == 3


def _greedy(ip, cap):
    """the rule in six lines: the longest run of consecutive patches that fits the cap, one patch above it on its own"""
    bounds, p0 = [0], 0
    while p0 < len(ip) - 1:
        p1 = p0 + 1
        while p1 < len(ip) - 1 and ip[p1 + 1] - ip[p0] <= cap:
            p1 += 1
        bounds.append(p1)
        p0 = p1
    return bounds


@pytest.mark.parametrize("npatch", [1, 2, 7, 40])
def test_range_planner(npatch):
    """plan_f32_ranges (csrc/patch_plan.h): the ranges an FP32 level of big patches is factored in"""
    sizes = np.random.default_rng(100 + npatch).integers(161, 401, npatch)
    pp = np.concatenate([[0], np.cumsum(sizes)])
    ip = _hostlib.plan_patch_layout(int(pp[-1]), pp, np.arange(pp[-1], dtype=np.int32))["inv_ptr"]
    doubles = np.diff(ip)
    k = min(npatch // 2, npatch - 2) if npatch > 1 else 0            # a patch with a right neighbour (where there is one)
    two = int(doubles[k] + doubles[k + 1]) if npatch > 1 else int(doubles[0])
    caps = [1, int(doubles[k]), two, two - 1, int(ip[-1]) + 1000]
    for cap in caps:
        plan = _hostlib.plan_f32_ranges(ip, cap)
        r = plan["ranges"]
        assert list(r) == _greedy(ip, cap), cap
        # a partition of [0, npatch) into non-empty ranges
        assert r[0] == 0 and r[-1] == npatch and np.all(np.diff(r) > 0)
        held = ip[r[1:]] - ip[r[:-1]]
        # every range is a single patch or fits the cap
        assert np.all((np.diff(r) == 1) | (held <= cap)), cap
        # no range could take the next patch
        assert all(ip[b + 1] - ip[a] > cap for a, b in zip(r[:-2], r[1:-1])), cap
        # the work buffer is the largest range
        assert plan["work_doubles"] == held.max(), cap
    assert len(_hostlib.plan_f32_ranges(ip, 1)["ranges"]) == npatch + 1            # one patch per range
    assert list(_hostlib.plan_f32_ranges(ip, caps[-1])["ranges"]) == [0, npatch]   # one range for the level
    empty = _hostlib.plan_f32_ranges(np.zeros(1, dtype=np.int64), 8)
    assert list(empty["ranges"]) == [0] and empty["work_doubles"] == 0
