"""Independent NumPy restatement of the SUPG and GLS residuals with a body force (alfi/stabilisation.py:47-97,
alfi/solver.py:204-217), written from the element tables only -- no call into the C++ pass it checks.

Per quadrature point, wt = w_q vol_c weight:
    Lu_k  = -nu (Lap u_k + d_k div u) + (u . grad) u_k - f_k
    beta  = (4 |u|^2 / h^2 + magic (4 nu / h^2)^2)^(-1/2)
    SUPG: F_(a,i) += wt beta Lu_i (u . grad phi_a)
    GLS:  F_(a,i) += wt beta [Lu_i (w . grad phi_a - nu Lap phi_a) - nu sum_k Lu_k d_k d_i phi_a]
"""
import numpy as np

from alfi_amd import _hostlib


def tables(V, nq=None):
    """Physical basis values, gradients and Hessians at the points of the SUPG rule in every cell."""
    lam, wq = _hostlib.supg_rule(V, nq)
    phi, dphi = V.element.tabulate(lam)                    # (nq, nloc), (nq, nloc, d+1)
    d2phi = V.element.tabulate_hessian(lam)                 # (nq, nloc, d+1, d+1)
    g, vol = V.mesh.cell_geometry()                         # (ncell, d+1, d): grad of the barycentric coordinates
    gp = np.einsum("qav,cvx->cqax", dphi, g)
    hs = np.einsum("qavw,cvx,cwy->cqaxy", d2phi, g, g)
    h = _hostlib.cell_size(V.mesh)
    return wq, phi, gp, hs, vol, h


def strong_residual(V, U, nu, fq=None, nq=None, tabs=None):
    """(u, Lu) at every point: (ncell, nq, d) each."""
    wq, phi, gp, hs, vol, h = tabs or tables(V, nq)
    Uc = np.asarray(U).reshape(-1, V.dim)[V.cell_nodes]     # (ncell, nloc, d)
    u = np.einsum("qa,cai->cqi", phi, Uc)
    Gu = np.einsum("cqax,cai->cqix", gp, Uc)
    lap = np.einsum("cqaxx->cqa", hs)
    Lu = -nu * np.einsum("cqa,cai->cqi", lap, Uc) - nu * np.einsum("cqajx,cax->cqj", hs, Uc) + np.einsum("cqx,cqix->cqi", u, Gu)
    if fq is not None:
        Lu = Lu - fq
    return u, Lu


def residual(kind, V, U, nu, weight, magic, W=None, fq=None, nq=None):
    """The stabilisation's residual contribution (num_dofs,) about U; kind "supg" or "gls" (wind W)."""
    tabs = tables(V, nq)
    wq, phi, gp, hs, vol, h = tabs
    d = V.dim
    u, Lu = strong_residual(V, U, nu, fq, tabs=tabs)
    h2 = (h * h)[:, None]
    beta = 1.0 / np.sqrt(4.0 * (u * u).sum(axis=2) / h2 + magic * (4.0 * nu / h2) ** 2)
    wt = wq[None, :] * vol[:, None] * weight
    c = (wt * beta)[:, :, None] * Lu                        # (ncell, nq, d)
    if kind == "supg":
        s = np.einsum("cqx,cqax->cqa", u, gp)
        Fe = np.einsum("cqi,cqa->cai", c, s)
    elif kind == "gls":
        Wc = np.asarray(W).reshape(-1, d)[V.cell_nodes]
        w = np.einsum("qa,cai->cqi", phi, Wc)
        t = np.einsum("cqx,cqax->cqa", w, gp) - nu * np.einsum("cqaxx->cqa", hs)
        Fe = np.einsum("cqi,cqa->cai", c, t) - nu * np.einsum("cqk,cqaki->cai", c, hs)
    else:
        raise ValueError(kind)
    F = np.zeros((V.num_nodes, d))
    np.add.at(F, V.cell_nodes, Fe)
    return F.ravel()
