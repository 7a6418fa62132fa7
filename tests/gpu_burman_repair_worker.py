"""Worker of tests/test_gpu_sv_p3_2d.py::test_flagged_patches_of_a_burman_level_are_repaired_with_the_facet_rule (own process:
the library reads ALFI_PATCH_CHECK_TOL once).  With a probe tolerance no inverse reaches, every macro star of the Burman-
stabilised [P3]^2 levels goes through the pivoted repair (kernels_check.hip: patch_repair_kernel), which must invert the matrix
PCPATCH assembles -- A[P, P] minus the facet terms of burman.patch_facet_corrections -- and not the plain sub-block.  Prints

    REPAIR <flagged> <repaired> <worst before> <worst after> ERR <largest error against np.linalg.inv> PLAIN <the same against
    the inverse of the uncorrected sub-block>"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from alfi_amd.burman import patch_facet_corrections
    from alfi_amd.nssolver import HipNavierStokesSolver
    from alfi_amd.problem import BSR, TwoDimLidDrivenCavityProblem
    s = HipNavierStokesSolver(TwoDimLidDrivenCavityProblem(2), 1, 3, discretisation="sv", stabilisation_type="burman",
                              stabilisation_weight=5e-3)
    d = 2
    u = np.random.default_rng(5).standard_normal(s.n_u)
    u[s.levels[-1].bc_dofs] = 0.0
    s.nu = 0.05
    s._device_states(u)
    L, dl, st, obj = s.levels[-1], s.hmg.mg.levels[-1], s._dstate[-1], s.hmg.pc_objs[-1]
    dl.assemble_burman(s.nu, s.gamma, 1.0, st, s.burman_weight, True)
    dl.factor()
    worst, flagged, repaired, after = dl.patch_check()
    A = BSR(L.A.nbrows, L.A.nbcols, d, L.A.rowptr, L.A.colidx,
            s.level_values(L, st.get().reshape(-1, d), 1.0, True)).to_scipy().tocsr()
    beta, scale = L.facet_beta
    ptr, col, fac, sv = patch_facet_corrections(L.V, L.facets, obj.patch_ptr, obj.patch_dofs)
    err = plain = 0.0
    for p in range(len(obj.patch_ptr) - 1):
        dofs = obj.patch_dofs[obj.patch_ptr[p]:obj.patch_ptr[p + 1]]
        n = dofs.size
        A0 = A[dofs][:, dofs].toarray()
        Ap = A0.copy()
        r0 = obj.patch_ptr[p] // d
        for i in range(n // d):
            for q in range(ptr[r0 + i], ptr[r0 + i + 1]):
                for c in range(d):
                    Ap[i * d + c, col[q] * d + c] -= scale * beta[fac[q]] * sv[q]
        X = dl.patch_inverse(p, n)
        ref, ref0 = np.linalg.inv(Ap), np.linalg.inv(A0)
        err = max(err, float(np.abs(X - ref).max() / np.abs(ref).max()))
        plain = max(plain, float(np.abs(X - ref0).max() / np.abs(ref0).max()))
    print("REPAIR %d %d %.3e %.3e ERR %.3e PLAIN %.3e NPATCH %d" % (flagged, repaired, worst, after, err, plain,
                                                                  len(obj.patch_ptr) - 1), flush=True)
    s.close()


if __name__ == "__main__":
    main()
