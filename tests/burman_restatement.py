"""Independent NumPy restatement of the Burman interior-penalty residual (alfi/stabilisation.py:139-162):

    R_B(u; v) = sum_F 0.5 weight avg(h)^2 beta_F(u) int_F jump(grad u, n) . jump(grad v, n) ds,
    beta_F(u) = |F|^-1 int_F sqrt(u.u + 1e-10) ds,  h^2 = |F|^2 (2-D) or |F| (3-D).

Facet by facet from the mesh alone: the quadrature points are placed on F in physical space, located in each of the two
cells by solving for their barycentric coordinates, and the gradients are evaluated there; the normal comes from the facet's
geometry.  It shares nothing with alfi_amd.burman but the element's tabulation and the name of the nonlinear rule
(burman.nonlinear_rule_points), and it never forms S_F."""
import numpy as np

from alfi_amd.burman import facet_rule, nonlinear_rule_points


def _bary(mesh, cell, x):
    X = mesh.coords[mesh.cells[cell]]                     # (d+1, d)
    T = (X[1:] - X[0]).T
    lr = np.linalg.solve(T, (x - X[0]).T).T               # (q, d)
    return np.concatenate([1.0 - lr.sum(axis=1, keepdims=True), lr], axis=1)


def _grad_basis(V, cell, lam):
    """Physical gradients (q, nloc, d) of the basis of ``cell`` at the barycentric points lam."""
    g, _ = V.mesh.cell_geometry()
    dphi = V.element.tabulate(lam)[1]                     # (q, nloc, d+1)
    return np.einsum("qai,ix->qax", dphi, g[cell])


def interior_facets(mesh):
    """(facet, cell0, cell1) for every interior facet, cell0 < cell1."""
    out = {}
    for c in range(mesh.num_cells):
        for f in mesh.cell_facets[c]:
            out.setdefault(int(f), []).append(c)
    return [(f, cs[0], cs[1]) for f, cs in sorted(out.items()) if len(cs) == 2]


def facet_geometry(mesh, f, kp):
    X = mesh.coords[mesh.facets[f]]                       # (d, d) vertices of F
    d = mesh.dim
    if d == 2:
        t = X[1] - X[0]
        area = np.linalg.norm(t)
        n = np.array([t[1], -t[0]]) / area
    else:
        c = np.cross(X[1] - X[0], X[2] - X[0])
        area = 0.5 * np.linalg.norm(c)
        n = c / np.linalg.norm(c)
    if n @ (X.mean(axis=0) - mesh.coords[mesh.cells[kp]].mean(axis=0)) < 0:
        n = -n                                            # out of K+
    return X, area, n


def residual(V, U, weight, facets=None):
    """R_B(U; phi_(a,i)) for every velocity dof, U (num_nodes, d)."""
    mesh, d = V.mesh, V.dim
    k = V.element.degree
    mu, w = facet_rule(d, nonlinear_rule_points(k))
    R = np.zeros((V.num_nodes, d))
    for f, kp, km in (facets if facets is not None else interior_facets(mesh)):
        X, area, n = facet_geometry(mesh, f, kp)
        x = mu @ X                                        # (q, d) points on F
        c = 0.5 * weight * (area ** 2 if d == 2 else area)
        lp, lm = _bary(mesh, kp, x), _bary(mesh, km, x)
        np_, nm = V.cell_nodes[kp], V.cell_nodes[km]
        phi = V.element.tabulate(lp)[0]
        u = phi @ U[np_]                                   # (q, d)
        beta = w @ np.sqrt((u * u).sum(axis=1) + 1e-10)
        dnp = _grad_basis(V, kp, lp) @ n                  # (q, nloc)
        dnm = _grad_basis(V, km, lm) @ n
        jump = dnp @ U[np_] - dnm @ U[nm]                 # (q, d): jump(grad u, n)
        wj = (c * beta * area * w)[:, None] * jump
        np.add.at(R, np_, dnp.T @ wj)
        np.add.at(R, nm, -(dnm.T @ wj))
    return R.ravel()
