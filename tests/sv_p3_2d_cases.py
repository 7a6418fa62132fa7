"""Shared by tests/test_sv_p3_2d.py (CPU) and tests/test_gpu_sv_p3_2d.py (-m gpu): the meshes of the 2-D [P3]^2-P2dg
Scott-Vogelius tests.  ldc2d with N = 2, and a 2 x 2 "union-jack" square whose centre vertex lies in 8 triangles -- its
macro star on the Alfeld-split mesh has 2 (9 + 64 + 24) = 194 dofs, beyond the register-resident patch path, while the
6-valent interior vertices of ldc2d give 2 (7 + 48 + 18) = 146.  Test infrastructure."""
import functools

import numpy as np

from alfi_amd.mesh import SimplexMesh
from alfi_amd.problem import TwoDimLidDrivenCavityProblem


class UnionJackCavityProblem(TwoDimLidDrivenCavityProblem):
    """The cavity problem on [0, 2]^2 cut into 8 triangles that all meet at the centre (vertex 4)."""

    def mesh(self, distribution_parameters=None):
        x = np.array([[i, j] for j in range(3) for i in range(3)], dtype=np.float64)
        ring = [0, 1, 2, 5, 8, 7, 6, 3]
        cells = [[4, ring[i], ring[(i + 1) % 8]] for i in range(8)]
        return SimplexMesh(x, np.array(cells, dtype=np.int32))


PROBLEMS = {"ldc2d": lambda: TwoDimLidDrivenCavityProblem(2), "unionjack": lambda: UnionJackCavityProblem(2)}


@functools.lru_cache(maxsize=None)
def hierarchy(mesh, nref, Re, gamma, advect=True, facet_coupling=False):
    """build_sv_hierarchy(k = 3) of one of the two meshes, built once per argument set; callers leave it unchanged."""
    from alfi_amd.sv import build_sv_hierarchy
    return build_sv_hierarchy(PROBLEMS[mesh](), nref, 3, Re=Re, gamma=gamma, advect=advect, facet_coupling=facet_coupling)
