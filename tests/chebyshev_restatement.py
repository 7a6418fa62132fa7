"""NumPy / SciPy restatement of the solver of the reference's grad-div experiment (examples/graddiv/graddiv.py:85-135): CG with
the unpreconditioned norm, preconditioned by one PCMG W-cycle whose level smoother is Chebyshev(2) around the additive patch
solves or point Jacobi.  Built on oracle.alfi_oracle (operators, patch smoother, Schoeberl transfer, V-cycle); what is new here:

* ``chebyshev``: Saad, Iterative Methods for Sparse Linear Systems, Alg. 12.1 on the preconditioned operator M A;
* ``arnoldi`` / ``chebyshev_bounds``: KSPChebyshevEstEigSet -- Ritz values of 10 Arnoldi steps on M A from
  ``default_rng(0).standard_normal(n)`` with the Dirichlet entries zeroed, interval (0.1, 1.1) x the largest real part;
* ``ChebyshevMultigrid``: PCMGMCycle_Private with ``cycles`` recursions on every level >= 2 (level 1 recurses once);
* ``cg``: KSPCG, zero initial guess, stopping on || r || <= rtol || b ||.

Test infrastructure only; the device path is checked against it (tests/test_gpu_chebyshev.py)."""
import functools

import numpy as np

from alfi_amd.problem import TwoDimLidDrivenCavityProblem, ThreeDimLidDrivenCavityProblem, build_hierarchy
from oracle import alfi_oracle as O

GAMMAS = (0.0, 1e2, 1e4, 1e6)
MAX_IT = 200
# the two small hierarchies of the experiment: name -> (problem, velocity degree, refinements)
CASES = {
    "2d": (lambda: TwoDimLidDrivenCavityProblem(4), 2, 2),      # [P2]^2 - P0, 3 levels, 2178 dofs
    "3d": (lambda: ThreeDimLidDrivenCavityProblem(2), 1, 1),    # [P1+FB]^3 - P0, 2 levels, 2967 dofs
}


class JacobiSmoother(object):
    """pc_type jacobi: y = x / diag(A), y = x on Dirichlet dofs."""

    def __init__(self, A, bc_dofs):
        self.diag, self.bc = A.diagonal().copy(), bc_dofs

    def apply(self, x):
        y = x / self.diag
        y[self.bc] = x[self.bc]
        return y


def chebyshev(A, M, b, x, k, emin, emax, nonzero_guess=True):
    """k steps of Saad's Alg. 12.1 for the interval [emin, emax] on M A.  A: matrix, M: callable.  Returns the new iterate."""
    theta, delta = 0.5 * (emax + emin), 0.5 * (emax - emin)
    sigma1 = theta / delta
    rho = 1.0 / sigma1
    x = x.copy() if nonzero_guess else np.zeros_like(b)
    d = None
    for i in range(k):
        z = M(b - A @ x)
        if i == 0:
            d = z / theta
        else:
            rho_new = 1.0 / (2.0 * sigma1 - rho)
            d = rho_new * rho * d + (2.0 * rho_new / delta) * z
            rho = rho_new
        x = x + d
    return x


def arnoldi(A, M, v0, m):
    """m Arnoldi steps (classical Gram-Schmidt) on M A from v0: the (m + 1) x m Hessenberg matrix."""
    n = v0.shape[0]
    V = np.zeros((m + 1, n))
    H = np.zeros((m + 1, m))
    V[0] = v0 / np.linalg.norm(v0)
    for j in range(m):
        w = M(A @ V[j])
        h = V[:j + 1] @ w
        w = w - h @ V[:j + 1]
        H[:j + 1, j] = h
        H[j + 1, j] = np.linalg.norm(w)
        V[j + 1] = w / H[j + 1, j]
    return H


def seed_vector(n, bc_dofs, seed=0):
    v = np.random.default_rng(seed).standard_normal(n)
    v[bc_dofs] = 0.0
    return v


def ritz_max(A, M, bc_dofs, steps=10, seed=0):
    """lambda: the largest real part of the Ritz values of ``steps`` Arnoldi steps on M A from the documented seed vector."""
    H = arnoldi(A, M, seed_vector(A.shape[0], bc_dofs, seed), steps)
    return float(np.linalg.eigvals(H[:steps, :steps]).real.max())


def chebyshev_bounds(A, M, bc_dofs, steps=10, seed=0):
    lam = ritz_max(A, M, bc_dofs, steps, seed)
    return 0.1 * lam, 1.1 * lam


class ChebyshevMultigrid(O.Multigrid):
    """oracle Multigrid with the Chebyshev(k) smoother and the M-cycle of PCMGMCycle_Private: level 1 visits the coarse solve
    once, every level >= 2 recurses ``cycles`` times on the same restricted right-hand side, continuing from the previous
    coarse iterate.  bounds[l] = (emin, emax) of level l (index 0 unused)."""

    def __init__(self, levels, transfers, k, bounds=None, cycles=2):
        O.Multigrid.__init__(self, levels, transfers, k)
        self.cycles = cycles
        self.bounds = bounds if bounds is not None else [None] + [
            chebyshev_bounds(L["A"], L["smoother"].apply, L["bc"]) for L in levels[1:]]

    def smooth(self, l, b, x):
        L = self.levels[l]
        return chebyshev(L["A"], L["smoother"].apply, b, x, self.k, *self.bounds[l])

    def vcycle(self, l, b, x):
        if l == 0:
            return self.coarse_lu.solve(b)
        x = self.smooth(l, b, x)
        r = b - self.levels[l]["A"] @ x
        bc = self.restrict(l, r)
        xc = np.zeros_like(bc)
        for _ in range(1 if l == 1 else self.cycles):
            xc = self.vcycle(l - 1, bc, xc)
        x = x + self.prolong(l, xc)
        return self.smooth(l, b, x)


def cg(A, M, b, rtol=1e-8, max_it=MAX_IT):
    """KSPCG, zero initial guess, unpreconditioned norm.  Returns (x, iterations, || r ||); iterations == max_it with
    || r || above the tolerance is the reference's ">200"."""
    x = np.zeros_like(b)
    r = b.copy()
    tol = rtol * np.linalg.norm(b)
    rn = np.linalg.norm(r)
    its, p, rz_old = 0, None, 0.0
    while rn > tol and its < max_it:
        z = M(r)
        rz = r @ z
        p = z if its == 0 else z + (rz / rz_old) * p
        w = A @ p
        alpha = rz / (p @ w)
        x = x + alpha * p
        r = r - alpha * w
        rz_old = rz
        rn = np.linalg.norm(r)
        its += 1
    return x, its, rn


def make_multigrid(lv, tr, smoother="patch", transfer=True, k=2, cycles=2):
    """The restatement's multigrid from the host generator's levels: ``smoother`` patch | jacobi; ``transfer`` False: the plain
    (bubble-corrected in 3-D) prolongation and its transpose instead of the Schoeberl pair."""
    mg = O.build_oracle_mg(lv, tr, k=k, schoeberl_restriction=True)
    if smoother == "jacobi":
        for L in mg.levels[1:]:
            L["smoother"] = JacobiSmoother(L["A"], L["bc"])
    if not transfer:
        for t in mg.transfers:
            P = t.st.P
            t.prolong = (lambda P: (lambda xc: P @ xc))(P)
            t.restrict = (lambda P: (lambda rf: P.T @ rf))(P)
    return ChebyshevMultigrid(mg.levels, mg.transfers, k, cycles=cycles)


@functools.lru_cache(maxsize=None)
def hierarchy(case, gamma):
    mk, k, nref = CASES[case]
    return build_hierarchy(mk(), nref, k, Re=0, gamma=gamma, advect=False)


@functools.lru_cache(maxsize=None)
def sv_hierarchy(gamma):
    """The smallest Scott-Vogelius hierarchy of the suite (macro-star patches, 2 levels)."""
    from alfi_amd.sv import build_sv_hierarchy
    return build_sv_hierarchy(TwoDimLidDrivenCavityProblem(2), 1, 2, Re=0, gamma=gamma, advect=False)


@functools.lru_cache(maxsize=None)
def multigrid(case, gamma, smoother="patch", transfer=True):
    lv, tr = sv_hierarchy(gamma) if case == "sv" else hierarchy(case, gamma)
    return make_multigrid(lv, tr, smoother, transfer)


def rhs(L):
    b = np.ones(L.n)
    b[L.bc_dofs] = 0.0
    return b


@functools.lru_cache(maxsize=None)
def solve(case, gamma, smoother="patch", transfer=True):
    """(iterations, || r ||, || b ||) of the experiment's solve: b = 1, b[bc] = 0, rtol 1e-8, at most 200 iterations."""
    lv, _ = sv_hierarchy(gamma) if case == "sv" else hierarchy(case, gamma)
    mg = multigrid(case, gamma, smoother, transfer)
    A, b = mg.levels[-1]["A"], rhs(lv[-1])
    top = len(mg.levels) - 1
    _, its, rn = cg(A, lambda r: mg.vcycle(top, r, np.zeros_like(r)), b)
    return its, rn, float(np.linalg.norm(b))
