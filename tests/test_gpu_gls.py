"""GLS stabilisation and the body force in the SUPG / GLS strong residual on the device (alfi_level_set_supg_load,
alfi_level_assemble_gls, alfi_level_gls) against the host pass, Newton with either assembly path, and the manufactured
solutions of examples/mms.py with SUPG and GLS: a residual-based stabilisation is consistent, so it keeps the unstabilised
orders (the thresholds of tests/test_gpu_mms.py) -- once the force is inside Lu.  -m gpu"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from alfi_amd.problem import TwoDimLidDrivenCavityProblem, ThreeDimLidDrivenCavityProblem

CASES = [("2d-P2", lambda: TwoDimLidDrivenCavityProblem(4), 2, 2), ("3d-P1FB", lambda: ThreeDimLidDrivenCavityProblem(2), 1, 1),
         ("3d-P2FB", lambda: ThreeDimLidDrivenCavityProblem(2), 2, 1)]


@pytest.mark.parametrize("name,mk,k,nref", CASES, ids=[c[0] for c in CASES])
def test_device_gls_terms_equal_the_host_pass(name, mk, k, nref):
    """Every level, random state, wind and load: the one-pass GLS refresh and the three-call sequence against the host pass,
    the residual contribution of GLS and of SUPG with the load; two refreshes (and several batches of cells) give the same bits."""
    from alfi_amd import _hostlib, hip
    from alfi_amd.nssolver import HipNavierStokesSolver
    s = HipNavierStokesSolver(mk(), nref, k, gamma=1e4, device_assembly=True, stabilisation_type="gls", stabilisation_weight=0.05)
    assert s.device_assembly and s.gls
    s.nu = 2.0 / 300.0
    rng = np.random.default_rng(17)
    s._fq = [None] * len(s.levels)
    s._host_winds = [None] * len(s.levels)
    for L, dl, st, dw in zip(s.levels, s.hmg.mg.levels, s._dstate, s._dwind):
        d = L.V.dim
        w = rng.standard_normal((L.V.num_nodes, d))
        W = rng.standard_normal((L.V.num_nodes, d))
        st.set(w.ravel())
        dw.set(W.ravel())
        s._host_winds[L.level] = W
        fq = hip.supg_load(L.V, lambda x: np.sin(x) + 0.3 * rng.standard_normal(x.shape))
        for load in (None, fq):
            s._fq[L.level] = load
            dl.set_supg_load(load)
            ref = s.level_values(L, w, 1.0, True)                   # host: assemble + gls + bc
            dl.assemble_gls(s.nu, s.gamma, 1.0, st, dw, s.supg_weight, s.supg_magic, True)
            one = dl.get_values()
            assert np.abs(one - ref).max() <= 1e-12 * np.abs(ref).max(), (name, L.level, load is None)
            dl.assemble_gls(s.nu, s.gamma, 1.0, st, dw, s.supg_weight, s.supg_magic, True)
            assert np.array_equal(one, dl.get_values())
            dl.assemble(s.nu, s.gamma, 1.0, st, False)              # the three-call sequence
            dl.gls(s.nu, s.supg_weight, s.supg_magic, st, dw, True, None)
            dl.apply_bc()
            assert np.abs(dl.get_values() - ref).max() <= 1e-12 * np.abs(ref).max(), (name, L.level)
            ndof = L.V.cell_nodes.shape[1] * d
            s.ctx.set_assembly_scratch(5 * ndof * ndof * 8 + 100)
            dl.assemble_gls(s.nu, s.gamma, 1.0, st, dw, s.supg_weight, s.supg_magic, True)
            assert np.array_equal(one, dl.get_values())
            s.ctx.set_assembly_scratch(24 << 30)
            for kind in ("gls", "supg"):
                Fh = np.zeros(L.n)
                dF = s.ctx.vec(L.n)
                if kind == "gls":
                    _hostlib.gls(L.V, w, W, s.nu, s.supg_weight, s.supg_magic, F=Fh, fq=load)
                    dl.gls(s.nu, s.supg_weight, s.supg_magic, st, dw, False, dF)
                else:
                    _hostlib.supg(L.V, w, s.nu, s.supg_weight, s.supg_magic, F=Fh, fq=load)
                    dl.supg(s.nu, s.supg_weight, s.supg_magic, st, False, dF)
                assert np.abs(dF.get() - Fh).max() <= 1e-12 * np.abs(Fh).max(), (name, L.level, kind, load is None)
        if load is not None:          # SUPG's linearisation with the load, one pass
            dl.assemble_supg(s.nu, s.gamma, 1.0, st, s.supg_weight, s.supg_magic, True)
            s.gls, s.supg = False, True
            host = s.level_values(L, w, 1.0, True)
            s.gls, s.supg = True, False
            assert np.abs(dl.get_values() - host).max() <= 1e-12 * np.abs(host).max(), (name, L.level)
    s.close()


def test_newton_with_gls_on_the_device_and_on_the_host_agree():
    from alfi_amd.nssolver import HipNavierStokesSolver, run_solver
    out = {}
    for dev in (True, False):
        s = HipNavierStokesSolver(ThreeDimLidDrivenCavityProblem(2), 2, 1, device_assembly=dev, stabilisation_type="gls",
                                  stabilisation_weight=0.05)
        res = run_solver(s, [10, 100])
        out[dev] = (s.u.copy(), [(res[r]["nonlinear_iter"], res[r]["linear_iter"], res[r]["converged"]) for r in (10, 100)])
        s.close()
    assert all(c for _, _, c in out[True][1]) and all(c for _, _, c in out[False][1])
    for (nd, ld, _), (nh, lh, _) in zip(out[True][1], out[False][1]):
        assert nd == nh and abs(ld - lh) <= 2, out
    assert np.abs(out[True][0] - out[False][0]).max() <= 1e-8 * np.abs(out[False][0]).max()


@pytest.mark.parametrize("stab,nrefs", [("supg", [1, 2, 3]), ("gls", [1, 2, 3, 4])])
def test_convergence_orders_2d(stab, nrefs):
    """[P2]^2-P0 with the 2-D default weight 1.  GLS's velocity order at Re 100 is still rising at nref 3 (1.72, 1.80: its
    test side adds the viscous operator of v, a larger perturbation on coarse meshes than SUPG's): one more refinement."""
    from mms import study
    from alfi_amd.mms import convergence_orders
    rates = {"velocity": 1.8, "velocitygrad": 0.85, "pressure": 0.85}
    hs, out = study(2, 4, nrefs, 2, "pkp0", [1.0, 100.0], verbose=False, stabilisation_type=stab)
    for re in (1.0, 100.0):
        for name, want in rates.items():
            orders = convergence_orders(out[re][name])
            assert orders[-1] > want, (stab, re, name, out[re][name], orders)


@pytest.mark.parametrize("stab", ["supg", "gls"])
def test_convergence_orders_3d_p1fb(stab):
    """The reference's mms3dpkp0 run line (examples/Makefile:19-21: [P1+FB]^3-P0 with SUPG), weight 0.05."""
    from mms import study
    from alfi_amd.mms import convergence_orders
    rates = {"velocity": 1.6, "velocitygrad": 0.9, "pressure": 0.9}
    hs, out = study(3, 2, [1, 2], 1, "pkp0", [1.0], verbose=False, stabilisation_type=stab, stabilisation_weight=0.05)
    for name, want in rates.items():
        orders = convergence_orders(out[1.0][name])
        assert orders[-1] > want, (stab, name, out[1.0][name], orders)
