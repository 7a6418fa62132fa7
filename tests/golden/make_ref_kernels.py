"""Recorded outputs of the reference's own C kernels (alfi/bubble.py split / splitadj / combine / combineadj / count, built
into oracle/_ref/ by oracle/build_ref.py) on the seeded inputs of tests/test_ref_kernels.py: the cell stencils applied to
one cell's arrays, and BubbleTransfer.prolong / .restrict driven cell by cell through the kernels on ldc3d [P1+FB]^3, two
levels, for seeds 1 and 2.  Data only, float64: the tests compare against it wherever the kernels cannot be built, and check
that the live kernels still reproduce it where they can.  Run from the repository root, with the reference tree present:
python tests/golden/make_ref_kernels.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    from tests.test_ref_kernels import RECORDED, load_reference_kernels, reference_kernel_outputs
    lib = load_reference_kernels()
    if lib is None:
        raise SystemExit("the reference kernels are not built (oracle/build_ref.py): nothing to record")
    out = reference_kernel_outputs(lib)
    np.savez_compressed(RECORDED, **out)
    print({k: (v.shape, float(np.linalg.norm(v))) for k, v in sorted(out.items())})


if __name__ == "__main__":
    main()
