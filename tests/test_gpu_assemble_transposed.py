"""The transposed operator refresh on serial levels (alfi_level_set_assembly_transposed; -m gpu): with the switch on, every
entry point that writes operator values from the device assembly writes A^T in the same sparsity, BITWISE what the forward
refresh followed by the in-place transpose (alfi_level_transpose, itself pinned bitwise to SciPy's transpose in
tests/test_gpu_adjoint.py) gives -- fused refreshes, the split sequences, cells in batches with both scratch layouts -- and
the forward refresh is back, bitwise, once it is off.  The solvers are those of tests/test_gpu_adjoint.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from alfi_amd import hip
from alfi_amd.nssolver import HipNavierStokesSolver
from alfi_amd.problem import BSR, TwoDimLidDrivenCavityProblem, ThreeDimLidDrivenCavityProblem

SOLVERS = {
    "pkp0-2d": lambda **kw: HipNavierStokesSolver(TwoDimLidDrivenCavityProblem(4), 1, 2, **kw),
    "pkp0-3d-k1": lambda **kw: HipNavierStokesSolver(ThreeDimLidDrivenCavityProblem(2), 1, 1, **kw),
    "pkp0-3d-k2": lambda **kw: HipNavierStokesSolver(ThreeDimLidDrivenCavityProblem(2), 1, 2, **kw),
    "supg-2d": lambda **kw: HipNavierStokesSolver(TwoDimLidDrivenCavityProblem(4), 1, 2, stabilisation_type="supg", **kw),
    "gls-2d": lambda **kw: HipNavierStokesSolver(TwoDimLidDrivenCavityProblem(4), 1, 2, stabilisation_type="gls",
                                                 stabilisation_weight=0.05, **kw),
    "sv-2d-burman": lambda **kw: HipNavierStokesSolver(TwoDimLidDrivenCavityProblem(2), 2, 2, discretisation="sv",
                                                       stabilisation_type="burman", stabilisation_weight=5e-3, **kw),
    "sv-3d-k3-burman": lambda **kw: HipNavierStokesSolver(ThreeDimLidDrivenCavityProblem(1), 1, 3, discretisation="sv",
                                                          stabilisation_type="burman", stabilisation_weight=5e-3, **kw),
}
ADV = 1.0


def _random_state(s, seed=0):
    """A non-trivial velocity on every level's state vector (and GLS's wind), nu = 0.02."""
    u = np.random.default_rng(seed).standard_normal(s.n_u)
    u[s.levels[-1].bc_dofs] = 0.0
    s.nu = 0.02
    s._device_states(u)
    if s.gls:
        s._device_winds()


def _mirror(rowptr, colidx):
    n = len(rowptr) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    key, mkey = rows * n + colidx, np.asarray(colidx, dtype=np.int64) * n + rows
    order = np.argsort(key)
    pos = np.searchsorted(key[order], mkey)
    assert np.array_equal(key[order][pos], mkey)
    return order[pos]


def _split_refresh(s, dl, st, wind):
    """The refresh in pieces: the cells' terms without boundary conditions, the stabilisation added to the operator, then the
    boundary conditions."""
    dl.assemble(s.nu, s.gamma, ADV, st, apply_bc=False)
    if s.supg:
        dl.supg(s.nu, s.supg_weight, s.supg_magic, st, True, None)
    if s.gls:
        dl.gls(s.nu, s.supg_weight, s.supg_magic, st, wind, True, None)
    if s.burman:
        dl.burman(ADV * s.burman_weight, st, True, None)
    dl.apply_bc()


def _forward_then_transpose(dl, refresh):
    refresh()
    v0 = dl.get_values()
    dl.transpose()
    return v0, dl.get_values()


def _transposed(dl, refresh):
    dl.set_assembly_transposed(True)
    try:
        refresh()
    finally:
        dl.set_assembly_transposed(False)
    return dl.get_values()


@pytest.mark.parametrize("case", list(SOLVERS))
def test_transposed_refresh_is_bitwise_refresh_then_transpose(case):
    s = SOLVERS[case]()
    try:
        assert s.device_assembly
        _random_state(s)
        groups = 0
        for L, (dl, st, wind) in zip(s.levels, s._device_levels()):
            fused = lambda: s._assemble_level(dl, st, wind, ADV)
            v0, vT = _forward_then_transpose(dl, fused)
            rp, ci = np.asarray(L.A.rowptr), np.asarray(L.A.colidx)
            assert np.array_equal(vT, np.transpose(v0[_mirror(rp, ci)], (0, 2, 1))), (case, L.level)     # the yardstick itself
            v1 = _transposed(dl, fused)
            assert np.array_equal(v1, vT), (case, L.level, float(np.abs(v1 - vT).max()))
            assert not np.array_equal(v1, v0)          # the operator is not symmetric: the switch did something
            fused()                                    # off again: the forward values, bit for bit
            assert np.array_equal(dl.get_values(), v0), (case, L.level)
            # the split sequence against ITS forward values transposed (the SUPG / GLS pieces are summed in another order
            # than in the fused refresh, forward and transposed alike)
            split = lambda: _split_refresh(s, dl, st, wind)
            w0, wT = _forward_then_transpose(dl, split)
            if not (s.supg or s.gls):
                assert np.array_equal(w0, v0) and np.array_equal(wT, vT), (case, L.level)
            w1 = _transposed(dl, split)
            assert np.array_equal(w1, wT), (case, L.level, float(np.abs(w1 - wT).max()))
            assert not np.array_equal(w1, w0)
            groups = max(groups, (dl.nnzb + 63) // 64)
        assert groups >= 4                             # several groups of 64 blocks of the lane-major layout
    finally:
        s.close()


@pytest.mark.parametrize("case", ["pkp0-2d", "supg-2d"])
def test_transposed_refresh_in_batches(case):
    """Cells in batches (the gather continues from the values in place), with the interleaved scratch layout ([P2]^2-P0) and
    the cell-contiguous one (SUPG): a scratch of a few cells, so that every level takes at least 3 batches, and one sized for
    a third of the finest level."""
    s = SOLVERS[case]()
    try:
        _random_state(s, seed=2)
        levels = list(zip(s.levels, s._device_levels()))
        yard = []
        for L, (dl, st, wind) in levels:
            yard.append(_forward_then_transpose(dl, lambda: s._assemble_level(dl, st, wind, ADV)))
        ndof = s.levels[-1].V.cell_nodes.shape[1] * s.levels[-1].bs
        per_cell = ndof * ndof * 8
        ncells = [L.V.mesh.num_cells for L in s.levels]
        for batch, which in (((min(ncells) - 1) // 3, levels), ((max(ncells) - 1) // 3, levels[-1:])):
            assert batch >= 1
            s.ctx.set_assembly_scratch(batch * per_cell)
            for (L, (dl, st, wind)), (v0, vT) in zip(which, yard[-len(which):]):
                assert -(-L.V.mesh.num_cells // batch) >= 3
                v1 = _transposed(dl, lambda: s._assemble_level(dl, st, wind, ADV))
                assert np.array_equal(v1, vT), (case, L.level, batch)
                s._assemble_level(dl, st, wind, ADV)
                assert np.array_equal(dl.get_values(), v0), (case, L.level, batch)
    finally:
        s.close()


def test_refused_without_an_assembly():
    ctx = hip.Context(0)
    try:
        vals = np.arange(1.0, 1.0 + 4 * 4).reshape(4, 2, 2)
        A = BSR(2, 2, 2, np.array([0, 2, 4], dtype=np.int32), np.array([0, 1, 0, 1], dtype=np.int32), vals)
        lv = hip.Level(ctx, A, np.zeros(0, dtype=np.int32))
        for on in (True, False):
            with pytest.raises(hip.AlfiHipError, match="error -2"):
                lv.set_assembly_transposed(on)
        assert np.array_equal(lv.get_values(), vals)
        lv.close()
    finally:
        ctx.close()
