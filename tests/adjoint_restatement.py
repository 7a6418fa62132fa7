"""NumPy / SciPy restatement of the adjoint of the Navier-Stokes Jacobian (alfi/solver.py:520-535) on a small 2-D problem,
assembled on the host: Newton with Reynolds continuation by direct solves, the adjoint by a direct solve of the transposed
Jacobian.  The pressure nullspace is handled by bordering: K x + (0, 1_p) s = b with vol . x_p = 0.  The right-hand side of the
adjoint comes from alfi_amd.adjoint.adjoint_rhs, so the sign, Dirichlet and nullspace conventions checked here are the ones the
device path uses."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from alfi_amd.adjoint import adjoint_rhs
from alfi_amd.mms import load_vector
from alfi_amd.nssolver import _assemble
from alfi_amd.problem import BSR, TwoDimLidDrivenCavityProblem, build_hierarchy, build_pressure_coupling


def force_shape(x):
    """The body force of amplitude 1 (the parameter m scales it)."""
    f = np.zeros_like(x)
    f[:, 0] = np.sin(np.pi * x[:, 1])
    f[:, 1] = x[:, 0] * (2.0 - x[:, 0])
    return f


class Restatement(object):
    """ldc2d, [P_k]^2 - P0, host operators of the finest level."""

    def __init__(self, baseN=4, nref=1, k=2, gamma=1e4):
        self.problem = TwoDimLidDrivenCavityProblem(baseN)
        lv, _ = build_hierarchy(self.problem, nref, k, Re=0.0, gamma=gamma, patches=False)
        self.L = L = lv[-1]
        self.gamma, self.d = gamma, L.bs
        self.B, self.B_raw, self.vol = build_pressure_coupling(L, both=True)
        self.n_u, self.n_p = L.n, self.B.shape[0]
        self.bc = L.bc_dofs
        self.u0 = np.zeros(self.n_u)
        bn = L.V.bc_nodes
        self.u0.reshape(-1, self.d)[bn] = self.problem.driver(L.V.node_coords[bn])
        self.load = load_vector(L.V, force_shape)
        self.nu0 = self.problem.char_length() * self.problem.char_velocity()

    def _mat(self, vals):
        L = self.L
        return BSR(L.A.nbrows, L.A.nbcols, L.bs, L.A.rowptr, L.A.colidx, vals).to_scipy()

    def residual(self, u, p, nu, m):
        """F(u, p; m) of solver.py:565-568 with the body force m * force_shape, Dirichlet rows zeroed (what nssolver forms)."""
        A0 = self._mat(_assemble(self.L, nu, self.gamma, 0.0, None, False))
        N = self._mat(_assemble(self.L, nu, self.gamma, 1.0, np.ascontiguousarray(u.reshape(-1, self.d)), False))
        Fu = 0.5 * (A0 @ u + N @ u) + self.B_raw.T @ p - m * self.load
        Fu[self.bc] = 0.0
        return np.concatenate([Fu, self.B_raw @ u])

    def jacobian(self, u, nu):
        """[[A, B^T], [B, 0]]: A with Dirichlet rows and columns identity, B with the Dirichlet columns zeroed."""
        A = self._mat(_assemble(self.L, nu, self.gamma, 1.0, np.ascontiguousarray(u.reshape(-1, self.d)), True))
        return sp.bmat([[A, self.B.T], [self.B, None]]).tocsr()

    def _bordered(self, K, b):
        n = K.shape[0]
        e = np.concatenate([np.zeros(self.n_u), np.ones(self.n_p)])
        w = np.concatenate([np.zeros(self.n_u), self.vol])
        M = sp.bmat([[K, sp.csr_matrix(e[:, None])], [sp.csr_matrix(w[None, :]), None]]).tocsc()
        return spla.spsolve(M, np.concatenate([b, [0.0]]))[:n]

    def solve(self, res, m, rtol=1e-12, max_it=30):
        """Newton with continuation over ``res``; returns (u, p, nu) of the last Re, p with zero integral."""
        u, p = self.u0.copy(), np.zeros(self.n_p)
        for re in res:
            nu = self.nu0 / re
            F = self.residual(u, p, nu, m)
            f0 = np.linalg.norm(F)
            for _ in range(max_it):
                if np.linalg.norm(F) <= rtol * f0:
                    break
                dz = self._bordered(self.jacobian(u, nu), -F)
                u, p = u + dz[:self.n_u], p + dz[self.n_u:]
                F = self.residual(u, p, nu, m)
        p = p - (self.vol @ p) / self.vol.sum()
        return u, p, nu

    def adjoint(self, u, nu, g_u, g_p):
        """lam = (lam_u, lam_p): J^T lam = -(g_u, g_p) projected by adjoint_rhs, lam_p with zero integral."""
        rhs = adjoint_rhs(g_u, g_p, self.bc, self.n_p, self.vol)
        lam = self._bordered(self.jacobian(u, nu).T.tocsr(), rhs)
        lam_u, lam_p = lam[:self.n_u], lam[self.n_u:]
        return lam_u, lam_p - (self.vol @ lam_p) / self.vol.sum(), rhs
