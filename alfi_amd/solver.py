"""Front end with the reference's plug-in surface for the velocity-block multigrid (alfi/solver.py).

* ``HipPatchPC``: a PCPython-protocol class (``initialize / update / apply / applyTranspose``; the in-tree example of
  that protocol is ``DGMassInv``, solver.py:15-38) that is selected exactly like the reference selects
  ``firedrake.PatchPC``: ``"pc_type": "python", "pc_python_type": "alfi_amd.HipPatchPC"`` (solver.py:318-319).  It reads
  the ``patch_pc_patch_*`` / ``patch_sub_*`` keys the reference sets (solver.py:320-344, 599-602) and runs PCPATCH's
  setup and apply on the GPU.
* ``mg_levels_solver`` / ``fieldsplit_0_mg``: the option dictionaries of ``get_parameters`` (solver.py:313-344, 359-379)
  with the PatchPC swapped for ``HipPatchPC``; ``fieldsplit_0_lu``: the exact velocity solve of solver_type allu
  (solver.py:346-352), the library's multifrontal factorisation of the finest operator.
* ``graddiv_solver`` / ``HipCG``: the solver of the reference's grad-div experiment (examples/graddiv/graddiv.py:85-135): CG
  preconditioned by one W-cycle with a Chebyshev(2) level smoother around the patch solves or point Jacobi.
* ``HipMG``: drives PCMG (full or multiplicative V / W) + FGMRES(k) or Chebyshev(k) from such a dictionary -- the stand-in for PETSc when
  petsc4py is not importable (it is not, in this image).  One ``apply`` = what ``fieldsplit_0``'s Richardson(1)/PCMG
  does to a right-hand side.
"""
import importlib

import numpy as np

from . import env, hip
from .relaxation import Options, PlexLike, patch_points_to_dofs

SUPPORTED_PATCH_KEYS = {
    "patch_pc_patch_save_operators", "patch_pc_patch_partition_of_unity", "patch_pc_patch_local_type",
    "patch_pc_patch_statistics", "patch_pc_patch_symmetrise_sweep", "patch_pc_patch_precompute_element_tensors",
    "patch_pc_patch_construct_type", "patch_pc_patch_construct_dim", "patch_pc_patch_construct_python_type",
    "patch_pc_patch_sub_mat_type", "patch_pc_patch_dense_inverse", "patch_pc_patch_multiplicative",
    "patch_sub_ksp_type", "patch_sub_pc_type", "patch_sub_pc_factor_mat_solver_type", "patch_pc_patch_sub_pc_type",
    "patch_pc_patch_condensed_sweeps",
}


def _truthy(v):
    return v if isinstance(v, bool) else str(v).lower() in ("1", "true", "yes")


def mg_levels_solver(tdim, patch="star", patch_composition="additive", smoothing=None, relaxation_direction=None,
                     condensed_sweeps=False):
    """The ``mg_levels_solver`` dictionary of alfi/solver.py:313-344 with ``configure_patch_solver`` of
    ConstantPressureSolver (solver.py:599-602) applied.  ``condensed_sweeps`` (this project's, not the reference's): emits
    ``patch_pc_patch_condensed_sweeps``, with which multiplicative sweeps read condensed patch factors (``HipPatchPC``)."""
    multiplicative = patch_composition == "multiplicative"
    if multiplicative and relaxation_direction is None:
        raise NotImplementedError("Need to specify a relaxation_direction in the problem.")
    if smoothing is None:
        smoothing = 10 if tdim > 2 else 6
    opts = {
        "ksp_type": "fgmres",
        "ksp_norm_type": "unpreconditioned",
        "ksp_max_it": smoothing,
        "ksp_convergence_test": "skip",
        "pc_type": "python",
        "pc_python_type": "alfi_amd.HipPatchPC",
        "patch_pc_patch_save_operators": True,
        "patch_pc_patch_partition_of_unity": False,
        "patch_pc_patch_local_type": "multiplicative" if multiplicative else "additive",
        "patch_pc_patch_statistics": False,
        "patch_pc_patch_symmetrise_sweep": multiplicative,
        "patch_pc_patch_precompute_element_tensors": True,
        "patch_sub_ksp_type": "preonly",
        "patch_sub_pc_type": "lu",
        "patch_pc_patch_sub_mat_type": "seqdense",
        "patch_sub_pc_factor_mat_solver_type": "petsc",
        "patch_pc_patch_dense_inverse": True,
    }
    if patch == "star":
        if multiplicative:
            opts["patch_pc_patch_construct_type"] = "python"
            opts["patch_pc_patch_construct_python_type"] = "alfi_amd.Star"
            opts["patch_pc_patch_construction_Star_sort_order"] = relaxation_direction
        else:
            opts["patch_pc_patch_construct_type"] = "star"
            opts["patch_pc_patch_construct_dim"] = 0
    elif patch == "macro":
        opts["patch_pc_patch_construct_type"] = "python"
        opts["patch_pc_patch_construct_python_type"] = "alfi_amd.MacroStar"
        opts["patch_pc_patch_construction_MacroStar_sort_order"] = relaxation_direction
    else:
        raise NotImplementedError("Unknown patch type %s" % patch)
    if condensed_sweeps:
        opts["patch_pc_patch_condensed_sweeps"] = True
    return opts


def configure_patch_solver_sv(opts, tdim, use_mkl=False):
    """ScottVogeliusSolver.configure_patch_solver (solver.py:655-659)."""
    opts = dict(opts)
    opts["patch_pc_patch_sub_mat_type"] = "seqaij"
    opts["patch_sub_pc_factor_mat_solver_type"] = ("mkl_pardiso" if use_mkl else "umfpack") if tdim > 2 else "petsc"
    opts.pop("patch_pc_patch_dense_inverse", None)
    return opts


def fieldsplit_0_mg(mg_levels):
    """alfi/solver.py:359-379 (the coarse solve is a dense inverse applied on the GPU instead of telescoped
    SuperLU_DIST; the keys are accepted and ignored)."""
    return {
        "ksp_type": "richardson",
        "ksp_richardson_self_scale": False,
        "ksp_max_it": 1,
        "ksp_norm_type": "unpreconditioned",
        "ksp_convergence_test": "skip",
        "pc_type": "mg",
        "pc_mg_type": "full",
        "pc_mg_log": None,
        "mg_levels": mg_levels,
        "mg_coarse_pc_type": "python",
        "mg_coarse_pc_python_type": "firedrake.AssembledPC",
        "mg_coarse_assembled": {"mat_type": "aij", "pc_type": "lu"},
    }


def fieldsplit_0_lu(use_mkl=False):
    """alfi/solver.py:346-352, key for key: fieldsplit_0 of solver_type allu (the ideal augmented-Lagrangian check).  The LU
    is the library's multifrontal factorisation of the finest operator (``hip.Saddle.factor_velocity``); the solver-package
    keys are accepted and ignored."""
    return {
        "ksp_type": "preonly",
        "ksp_max_it": 1,
        "pc_type": "lu",
        "pc_factor_mat_solver_type": "mkl_pardiso" if use_mkl else "mumps",
        "mat_mumps_icntl_14": 150,
    }


def is_fieldsplit_0_lu(params):
    """Whether a fieldsplit_0 dictionary asks for the exact velocity solve (preonly + pc_type lu)."""
    return params.get("pc_type") == "lu" and params.get("ksp_type") == "preonly"


def graddiv_solver(smoother="patch", patch="star"):
    """The solver dictionary of the reference's grad-div experiment (examples/graddiv/graddiv.py:85-135), key for key, with
    the ``mg_levels_`` keys nested under ``mg_levels`` and the PatchPC / MacroStar classes swapped for this package's: CG
    (rtol 1e-8, at most 200 iterations, unpreconditioned norm) preconditioned by one PCMG W-cycle whose level smoother is
    Chebyshev(2) around ``smoother`` = "patch" (additive ``patch`` = "star" or "macro" patches) or "jacobi"."""
    sp = {
        "mat_type": "aij",
        "snes_type": "ksponly",
        "ksp_type": "cg",
        "ksp_rtol": 1e-8,
        "ksp_atol": 0,
        "ksp_max_it": 200,
        "ksp_norm_type": "unpreconditioned",
        "pc_type": "mg",
        "pc_mg_cycle_type": "w",
        "mg_coarse_ksp_type": "preonly",
        "mg_coarse_pc_type": "python",
        "mg_coarse_pc_python_type": "firedrake.AssembledPC",
        "mg_coarse_assembled_pc_type": "lu",
        "mg_coarse_assembled_pc_factor_mat_solver_type": "superlu_dist",
    }
    mgl = {"ksp_type": "chebyshev", "ksp_max_it": 2}
    if smoother == "patch":
        mgl.update({
            "pc_type": "python",
            "pc_python_type": "alfi_amd.HipPatchPC",
            "patch_pc_patch_save_operators": True,
            "patch_pc_patch_partition_of_unity": False,
            "patch_pc_patch_multiplicative": False,
            "patch_pc_patch_symmetrise_sweep": False,
            "patch_sub_ksp_type": "preonly",
            "patch_sub_pc_type": "lu",
        })
        if patch == "macro":
            mgl.update({
                "patch_pc_patch_construct_type": "python",
                "patch_pc_patch_construct_python_type": "alfi_amd.MacroStar",
                "patch_pc_patch_sub_mat_type": "aij",
                "patch_pc_patch_sub_pc_type": "lu",
                "patch_sub_pc_factor_mat_solver_type": "umfpack",
            })
        elif patch == "star":
            mgl.update({
                "patch_pc_patch_construct_type": "star",
                "patch_pc_patch_construct_dim": 0,
                "patch_pc_patch_sub_mat_type": "dense",
            })
        else:
            raise NotImplementedError("Unknown patch type %s" % patch)
    elif smoother == "jacobi":
        mgl["pc_type"] = "jacobi"
    else:
        raise NotImplementedError("smoother %r (patch or jacobi; the reference's amg column is hypre)" % (smoother,))
    sp["mg_levels"] = mgl
    return sp


BUILT_SMOOTHERS = ("fgmres", "chebyshev")


def parse_mg_options(params):
    """What ``HipMG`` reads from a ``pc_type mg`` dictionary, checked without touching a device: dict(smoother, k, pc, full,
    cycle, esteig, esteig_steps, eigenvalues)."""
    if params.get("pc_type") != "mg":
        raise ValueError("expected the fieldsplit_0_mg dictionary (pc_type mg)")
    mgl = params["mg_levels"]
    ksp = mgl.get("ksp_type")
    if ksp not in BUILT_SMOOTHERS:
        raise NotImplementedError("level smoother ksp_type %r: built are %s" % (ksp, ", ".join(BUILT_SMOOTHERS)))
    if ksp == "fgmres" and mgl.get("ksp_convergence_test") != "skip":
        raise NotImplementedError("level smoother must be fgmres with convergence_test skip (solver.py:314-317)")
    pc = mgl.get("pc_type")
    if pc not in ("python", "jacobi"):
        raise NotImplementedError("level pc_type must be python or jacobi")
    cycle = str(params.get("pc_mg_cycle_type", "v")).lower()
    if cycle not in ("v", "w"):
        raise NotImplementedError("pc_mg_cycle_type %r (v or w)" % (cycle,))
    out = {"smoother": ksp, "k": int(mgl["ksp_max_it"]), "pc": pc, "cycle": cycle,
           "full": params.get("pc_mg_type", "multiplicative") == "full",
           "esteig": None, "esteig_steps": None, "eigenvalues": None}
    if ksp == "chebyshev":
        def numbers(key, default, count):
            text = str(mgl.get(key, default))
            try:
                vals = tuple(float(t) for t in text.split(","))
            except ValueError:
                raise ValueError("%s: %r is not a comma-separated list of numbers" % (key, text))
            if len(vals) != count:
                raise ValueError("%s: %r must hold %d numbers" % (key, text, count))
            return vals
        out["esteig"] = numbers("ksp_chebyshev_esteig", "0,0.1,0,1.1", 4)
        out["esteig_steps"] = int(mgl.get("ksp_chebyshev_esteig_steps", 10))
        if not 1 <= out["esteig_steps"] <= 30:
            raise ValueError("ksp_chebyshev_esteig_steps %d not in 1..30" % out["esteig_steps"])
        if mgl.get("ksp_chebyshev_eigenvalues") is not None:
            emin, emax = numbers("ksp_chebyshev_eigenvalues", None, 2)
            if not 0.0 < emin < emax:
                raise ValueError("ksp_chebyshev_eigenvalues: need 0 < emin < emax, got %r" % (mgl["ksp_chebyshev_eigenvalues"],))
            out["eigenvalues"] = (emin, emax)
    return out


def _resolve(dotted):
    mod, _, name = dotted.rpartition(".")
    return getattr(importlib.import_module(mod), name)


def macro_vertex_labels(mesh):
    """``MacroVertices`` label (alfi/bary.py:18-19 sets it to 1 on the vertices of the mesh that is then split).  For a
    uniformly refined mesh the analogous macro vertices are the vertices inherited from the parent mesh; a mesh without
    parent information carries no label."""
    if getattr(mesh, "macro_vertex_mask", None) is not None:          # Alfeld split (mesh.bary_refine): the split mesh's vertices
        return {"MacroVertices": {int(mesh.num_cells + v): 1 for v in np.flatnonzero(mesh.macro_vertex_mask)}}
    if getattr(mesh, "vertex_parents", None) is None:
        return {}
    vp_ = np.asarray(mesh.vertex_parents)
    macro = np.flatnonzero(vp_[:, 0] == vp_[:, 1])
    nc = mesh.num_cells
    return {"MacroVertices": {int(nc + v): 1 for v in macro}}


class PC(object):
    """The small part of a PETSc PC object a PCPython class touches: operators, DM, options prefix (+ attributes)."""

    def __init__(self, ctx, level_data, options=None, prefix=""):
        self.ctx = ctx                  # alfi_amd.hip.Context
        self.level_data = level_data    # alfi_amd.problem.LevelData (operator, space, Dirichlet dofs)
        self.options = dict(options or {})
        self.prefix = prefix
        self._dm = PlexLike(level_data.V.mesh, labels=macro_vertex_labels(level_data.V.mesh))
        self.attrs = {}

    def getOperators(self):
        return self.level_data.A, self.level_data.A

    def getDM(self):
        return self._dm

    def getOptionsPrefix(self):
        return self.prefix

    def getAttr(self, k):
        return self.attrs.get(k)

    def setAttr(self, k, v):
        self.attrs[k] = v


def _as_device(ctx, v, n):
    """(DeviceVec, writeback) for a DeviceVec, a NumPy array, or anything with getArray() (petsc4py Vec)."""
    if isinstance(v, hip.DeviceVec):
        return v, None
    arr = v.getArray() if hasattr(v, "getArray") else v
    arr = np.asarray(arr)
    assert arr.shape == (n,)
    return ctx.vec(arr), arr


def _dense_array(M):
    """The (n, ncol) array behind a dense operand of ``matApply``: a NumPy array, or anything with getDenseArray() (a
    petsc4py dense Mat, one column per right-hand side)."""
    return np.asarray(M.getDenseArray() if hasattr(M, "getDenseArray") else M)


def check_mat_apply_args(X, Y, n):
    """The operands of a ``matApply(pc, X, Y)`` (PETSc's PCMatApply, which KSPMatSolve calls): dense, one column of n
    entries per right-hand side, as many columns in Y as in X, X and Y distinct.  Each is a hip.DeviceMat or a host array
    (``_dense_array``).  ValueError before anything touches the device; returns the number of columns."""
    shapes = []
    for name, M in (("X", X), ("Y", Y)):
        if isinstance(M, hip.DeviceMat):
            shapes.append((M.n, M.ncol))
            continue
        a = _dense_array(M)
        if a.ndim != 2 or a.dtype != np.float64:
            raise ValueError("matApply: %s must be a dense float64 matrix with one column per right-hand side, got %s %s"
                             % (name, a.dtype, a.shape))
        shapes.append(a.shape)
    if X is Y or (not isinstance(X, hip.DeviceMat) and not isinstance(Y, hip.DeviceMat)
                  and np.shares_memory(_dense_array(X), _dense_array(Y))):
        raise ValueError("matApply: X and Y must not alias")
    for name, s in zip("XY", shapes):
        if s[0] != n or s[1] < 1:
            raise ValueError("matApply: %s is %d x %d, expected %d rows and at least one column" % (name, s[0], s[1], n))
    if shapes[0][1] != shapes[1][1]:
        raise ValueError("matApply: X has %d columns, Y has %d" % (shapes[0][1], shapes[1][1]))
    if not isinstance(Y, hip.DeviceMat) and not _dense_array(Y).flags.writeable:
        raise ValueError("matApply: Y is read-only")
    return shapes[0][1]


def _as_device_mat(ctx, M):
    """(DeviceMat, writeback) for a checked operand of ``matApply``"""
    if isinstance(M, hip.DeviceMat):
        return M, None
    a = _dense_array(M)
    return ctx.mat(a), a


class HipPatchPC(object):
    """PCPATCH on the GPU behind the PCPython protocol (solver.py:15-38 shows the protocol)."""

    def initialize(self, pc):
        opts = Options(pc.getOptionsPrefix(), pc.options)
        L = pc.level_data
        unknown = [k for k in pc.options if k.startswith(pc.getOptionsPrefix() + "patch_")
                   and k[len(pc.getOptionsPrefix()):] not in SUPPORTED_PATCH_KEYS
                   and "patch_pc_patch_construction_" not in k]
        if unknown:
            raise ValueError("unsupported PatchPC options: %s" % unknown)
        local_type = opts.getString("patch_pc_patch_local_type", "additive")
        if _truthy(opts.getString("patch_pc_patch_multiplicative", "false")):
            local_type = "multiplicative"
        if local_type not in ("additive", "multiplicative"):
            raise NotImplementedError("patch local_type %r" % local_type)
        self.multiplicative = local_type == "multiplicative"
        self.symmetrise = _truthy(opts.getString("patch_pc_patch_symmetrise_sweep", "false"))
        self.partition_of_unity = _truthy(opts.getString("patch_pc_patch_partition_of_unity", "false"))
        if self.partition_of_unity and self.multiplicative:
            raise NotImplementedError("partition_of_unity with multiplicative sweeps")
        if self.multiplicative and getattr(L, "facet_coupling", False):
            raise NotImplementedError("multiplicative patch sweeps on a facet-coupled (Burman) level: the sweep's dependency "
                                      "waves assume cell coupling")
        sub_mat = opts.getString("patch_pc_patch_sub_mat_type", "seqdense")
        if sub_mat not in ("seqdense", "dense", "seqaij", "aij"):
            raise NotImplementedError("patch sub_mat_type %r" % sub_mat)
        # seqaij (ScottVogeliusSolver.configure_patch_solver, solver.py:655-659: sparse patch matrices factored by
        # UMFPACK / PARDISO) asks for the same operator A_p^-1 as seqdense + dense_inverse (solver.py:599-602); here both
        # are the explicit dense inverse -- macro-star patches are inverted on the FP64 matrix cores
        ctype = opts.getString("patch_pc_patch_construct_type", "star")
        cdim = opts.getInt("patch_pc_patch_construct_dim", 0)
        ctor = None
        if ctype == "star" and cdim == 0:
            ptr, dofs, _ = L.V.star_patches()
            self.iterset = np.arange(len(ptr) - 1)
        elif ctype in ("star", "python"):
            if ctype == "star":
                # built-in stars of edges / faces / cells (patch_pc_patch_construct_dim != 0; the reference passes 0,
                # solver.py:338): the same point sets as the python Star constructor seeded on that stratum
                from .relaxation import Star
                ctor = Star()
                pc.options = dict(pc.options)
                pc.options[pc.getOptionsPrefix() + "patch_pc_patch_construction_Star_dim"] = cdim
            else:
                ctor = _resolve(opts.getString("patch_pc_patch_construct_python_type"))()
            # firedrake.PatchPC hands the constructor its inner PCPATCH object, whose options prefix is the outer one
            # + "patch_" [3P]: that is where pc_patch_construction_<Name>_sort_order lives (solver.py:335, 342)
            inner = PC(pc.ctx, pc.level_data, options=pc.options, prefix=pc.getOptionsPrefix() + "patch_")
            inner._dm = pc.getDM()
            patches, iterset = ctor(inner)
            ptr, dofs, kept = patch_points_to_dofs(L.V, pc.getDM(), patches)
            # the iteration set indexes the constructor's patch list; patches without free dofs were dropped (PCPATCH
            # skips them in the sweep: `if (len <= 0) continue` [3P])
            new = np.full(len(patches), -1, dtype=np.int64)
            new[np.asarray(kept, dtype=np.int64)] = np.arange(len(kept))
            it = new[np.asarray(iterset, dtype=np.int64)]
            self.iterset = it[it >= 0]
        else:
            raise NotImplementedError("patch construct_type %r" % ctype)
        self.patch_ptr, self.patch_dofs = ptr, dofs
        self.level = hip.Level(pc.ctx, L.A, L.bc_dofs)
        self.level.set_patches(ptr, dofs)
        # macro-star patches on an Alfeld-split mesh (ScottVogeliusSolver: the reference keeps SPARSE patch factors there,
        # solver.py:655-659): store the factors condensed -- interiors of the macro cells + skeleton -- unless the sweep is
        # multiplicative (that kernel multiplies with dense inverses) and patch_pc_patch_condensed_sweeps is not set
        self.condensed = False
        # opt-in: multiplicative sweeps that read condensed factors (hip.Level.set_multiplicative(..., condensed=True))
        self.condensed_sweeps = self.multiplicative and _truthy(opts.getString("patch_pc_patch_condensed_sweeps", "false"))
        if (ctype == "python" and getattr(L.V.mesh, "macro_mesh", None) is not None
                and (not self.multiplicative or self.condensed_sweeps)
                and env.condense() and type(ctor).__name__ == "MacroStar"
                and ctype == "python" and not getattr(L, "facet_coupling", False)):
            # (not on facet-coupled levels: the Burman term couples the interiors of neighbouring macro cells)
            from .sv import macro_cell_groups
            self.level.set_patch_groups(macro_cell_groups(L.V, dofs))
            self.condensed = True
        elif (self.condensed_sweeps and env.condense() and ctype == "star" and cdim == 0
              and not getattr(L, "facet_coupling", False)):
            # built-in vertex stars: the groups the level finds in its own sparsity, handed back as the caller's -- a level
            # that condensed itself would go back to dense inverses for the sweeps
            groups = self.level.find_patch_groups()
            if (groups >= 0).any():
                self.level.set_patch_groups(groups)
                self.condensed = True
            else:
                self.level.set_patch_groups(None)
        elif self.multiplicative or not env.condense() or getattr(L, "facet_coupling", False):
            # ... and no search for groups by the level itself either (large vertex-star levels, alfi_patches_find_groups):
            # the sweeps and PCPATCH's facet rule need dense inverses, ALFI_CONDENSE=0 asks for them
            self.level.set_patch_groups(None)
        # (operator values not there yet -- formed on the device by the caller, who then factors: problem.build_hierarchy
        # with operator_values=False)
        # the front end's patch_factor_dtype (HipMG hands it over as an attribute of the PC).  Not asked where this class sets
        # multiplicative sweeps or the caller a facet correction afterwards: neither has an FP32 form, the level keeps FP64
        if not self.multiplicative and not getattr(L, "facet_coupling", False):
            hip.ask_patch_storage(self.level, getattr(pc, "patch_factor_dtype", None))
        # the front end's macro_factor_dtype: asked after the groups decision, facet-coupled levels included (the request takes a
        # facet correction set afterwards).  A level that got the caller's groups above is refused and stays condensed FP64.
        if not self.multiplicative:
            hip.ask_macro_patch_storage(self.level, getattr(pc, "macro_factor_dtype", None))
        if L.A.vals is not None:
            self.level.factor()
        hip.note_patch_level(L, self.level)
        if self.partition_of_unity:
            self.level.set_partition_of_unity(True)
        self.wavefronts = (self.level.set_multiplicative(self.iterset, self.symmetrise, condensed=self.condensed_sweeps)
                           if self.multiplicative else 0)
        self.n = L.n

    def update(self, pc):
        """New operator values (Newton step / Reynolds continuation): re-gather and re-invert every patch, which is what
        PatchPC.update -> PCSetUp_PATCH does with save_operators (solver.py:320)."""
        self.level.update_values(pc.level_data.A.vals)
        fb = getattr(pc.level_data, "facet_beta", None)     # host-assembled Burman values: beta_F and the term's weight
        if fb is not None:
            self.level.set_facet_beta(*fb)
        self.level.factor()

    def apply(self, pc, x, y):
        dx, _ = _as_device(pc.ctx, x, self.n)
        dy, ywb = _as_device(pc.ctx, y, self.n)
        self.level.patch_apply(dx, dy)
        if ywb is not None:
            ywb[:] = dy.get()

    def matApply(self, pc, X, Y):
        """PCMatApply: ``apply`` on every column of the dense X into the same column of Y (hip.Level.patch_apply_block: the
        patch factors are streamed once for up to four columns where the level batches)."""
        check_mat_apply_args(X, Y, self.n)
        dX, _ = _as_device_mat(pc.ctx, X)
        dY, ywb = _as_device_mat(pc.ctx, Y)
        self.level.patch_apply_block(dX, dY)
        if ywb is not None:
            ywb[...] = dY.get()

    def applyTranspose(self, pc, x, y):
        raise NotImplementedError("Sorry!")


class HipMG(object):
    """PCMG + KSPFGMRES(k) or KSPCHEBYSHEV(k) driven by the reference's option dictionary (solver.py:359-379,
    examples/graddiv/graddiv.py:99-139), device resident.  ``mg_levels``: ``ksp_type`` fgmres | chebyshev with ``ksp_max_it``;
    for chebyshev ``ksp_chebyshev_esteig`` ("a,b,c,d", default "0,0.1,0,1.1"), ``ksp_chebyshev_esteig_steps`` (default 10) or
    ``ksp_chebyshev_eigenvalues`` ("emin,emax": no estimate is run); ``pc_type`` python (``pc_python_type``) | jacobi.
    ``pc_mg_cycle_type`` v | w.  The Chebyshev intervals are estimated at construction and again by ``update``."""

    def __init__(self, ctx, levels, transfers, params, restriction=False, coarse_inv=None, patch_factor_dtype=None,
                 macro_factor_dtype=None):
        """patch_factor_dtype: None, or "f32": every smoothed level is asked to store its dense patch inverses in single
        precision (hip.ask_patch_storage; a keyword, not an option: the dictionaries mirror the reference's).
        macro_factor_dtype: None, or "f32": the same request in the form macro stars and Burman levels can take
        (hip.ask_macro_patch_storage: levels with the caller's groups stay condensed FP64).  One of the two at most."""
        hip.check_factor_dtypes(patch_factor_dtype, macro_factor_dtype)
        self.opts = o = parse_mg_options(params)
        mgl = params["mg_levels"]
        self.k = o["k"]
        self.full = o["full"]
        jacobi = o["pc"] == "jacobi"
        pc_cls = None if jacobi else _resolve(mgl["pc_python_type"])
        self.ctx = ctx
        self.pcs, self.pc_objs = [], []
        dlevels = []
        for L in levels:
            if L.level == 0:
                dl = hip.Level(ctx, L.A, L.bc_dofs)
                if coarse_inv is not None:
                    dl.set_coarse_inverse(coarse_inv)
                elif L.A.vals is None:      # values formed on the device later: remember the choice, factor then
                    dl._coarse_choice = ("auto", None)
                else:
                    dl.coarse_factor_auto(getattr(getattr(L, "V", None), "node_coords", None))
                dlevels.append(dl)
                self.pcs.append(None)
                self.pc_objs.append(None)
                continue
            pc = PC(ctx, L, options=mgl)
            pc.patch_factor_dtype = patch_factor_dtype
            pc.macro_factor_dtype = macro_factor_dtype
            obj = HipJacobiPC() if jacobi else pc_cls()
            obj.initialize(pc)
            self.pcs.append(pc)
            self.pc_objs.append(obj)
            dlevels.append(obj.level)
        self.mg = hip.Multigrid.__new__(hip.Multigrid)
        hip.Multigrid._from_device_levels(self.mg, ctx, dlevels, transfers, self.k, restriction)
        self.n = levels[-1].n
        if o["cycle"] != "v":
            self.mg.set_cycle_type(o["cycle"])
        self.bounds = None
        if o["smoother"] == "chebyshev":
            self._set_chebyshev()

    def _set_chebyshev(self):
        o = self.opts
        if o["eigenvalues"] is not None:
            self.bounds = [o["eigenvalues"]] * (len(self.mg.levels) - 1)
        else:
            self.bounds = self.mg.chebyshev_bounds(o["esteig_steps"], o["esteig"])
        self.mg.set_smoother("chebyshev", self.bounds)

    def update(self, levels):
        for pc, obj, L in zip(self.pcs, self.pc_objs, levels):
            if obj is not None:
                pc.level_data = L
                obj.update(pc)
        if self.opts["smoother"] == "chebyshev":       # the intervals belong to the old operators and patch factors
            self._set_chebyshev()

    def apply(self, b, x):
        """x <- PCMG(b): one full cycle (pc_mg_type full) or one V-cycle from a zero initial guess."""
        db, _ = _as_device(self.ctx, b, self.n)
        dx, xwb = _as_device(self.ctx, x, self.n)
        if self.full:
            self.mg.fcycle(db, dx)
        else:
            dx.zero()
            self.mg.vcycle(db, dx)
        if xwb is not None:
            xwb[:] = dx.get()

    def matApply(self, B, X):
        """``apply`` on every column of the dense B into the same column of X (PCMatApply's shape; hip.Multigrid.fcycle_block /
        vcycle_block)."""
        check_mat_apply_args(B, X, self.n)
        dB, _ = _as_device_mat(self.ctx, B)
        dX, xwb = _as_device_mat(self.ctx, X)
        if self.full:
            self.mg.fcycle_block(dB, dX)
        else:
            dX.zero()
            self.mg.vcycle_block(dB, dX)
        if xwb is not None:
            xwb[...] = dX.get()


class HipJacobiPC(object):
    """``pc_type jacobi`` on a level (examples/graddiv/graddiv.py:137-139) behind the same protocol: y = x / diag(A), y = x on
    Dirichlet dofs.  No patches, no factorisation."""

    def initialize(self, pc):
        L = pc.level_data
        self.level = hip.Level(pc.ctx, L.A, L.bc_dofs)
        self.level.set_jacobi(True)
        self.n = L.n

    def update(self, pc):
        self.level.update_values(pc.level_data.A.vals)

    def apply(self, pc, x, y):
        dx, _ = _as_device(pc.ctx, x, self.n)
        dy, ywb = _as_device(pc.ctx, y, self.n)
        self.level.patch_apply(dx, dy)
        if ywb is not None:
            ywb[:] = dy.get()

    def applyTranspose(self, pc, x, y):
        self.apply(pc, x, y)


class HipCG(object):
    """The reference's grad-div solve on the GPU (examples/graddiv/graddiv.py:85-135, 155-172): KSPCG with a zero initial
    guess and the unpreconditioned norm around one PCMG cycle (``HipMG``), driven by the ``graddiv_solver`` dictionary.
    ``transfer``: the Schoeberl prolongation and restriction (the reference's ``--transfer``); False: the plain nodal
    (bubble-corrected in 3-D) prolongation P and its transpose -- the same device transfer with gamma = 0 in its interior
    solves, which makes both directions exactly P and P^T (the non-robust restriction would be the transpose of the PLAIN
    nodal interpolation, which differs from P^T for the bubble-corrected 3-D pair and would leave CG an unsymmetric
    preconditioner).  ``solve(b) -> (x, iterations, residual norm)``; iterations =
    ``ksp_max_it`` means the solve did not converge."""

    def __init__(self, ctx, levels, transfers, params, transfer=True):
        if params.get("ksp_type") != "cg" or params.get("ksp_norm_type", "unpreconditioned") != "unpreconditioned":
            raise NotImplementedError("outer solver must be cg with the unpreconditioned norm (graddiv.py:88, 94)")
        self.ctx, self.transfer = ctx, bool(transfer)
        self.rtol, self.atol = float(params.get("ksp_rtol", 1e-5)), float(params.get("ksp_atol", 1e-50))
        self.max_it = int(params.get("ksp_max_it", 10000))
        self.hmg = HipMG(ctx, levels, transfers, params, restriction=True)
        self.mg = self.hmg.mg
        self._transfers = list(transfers)
        self._plain_transfers()
        self.n = levels[-1].n
        self._b, self._x = ctx.vec(self.n), ctx.vec(self.n)

    def _plain_transfers(self):
        # prolong (I - gamma E inv(A_II) E^T D) P and restrict P^T (I - gamma D E inv(A_II) E^T) at gamma = 0: P and P^T
        if not self.transfer:
            for dt, T in zip(self.mg.transfers, self._transfers):
                dt.update(T.nu, 0.0)

    def update(self, levels, transfers=None):
        """New operator values on every level (a new gamma): patch factors, Chebyshev intervals and -- with ``transfers``, the
        new TransferData -- the interior solves of the Schoeberl transfer."""
        if transfers is not None:
            self._transfers = list(transfers)
            for dt, T in zip(self.mg.transfers, self._transfers):
                dt.update(T.nu, T.gamma if self.transfer else 0.0)
        L0 = self.mg.levels[0]
        L0.update_values(levels[0].A.vals)
        L0.coarse_factor_auto()
        self.hmg.update(levels)

    def solve(self, b, x=None):
        self._b.set(np.asarray(b, dtype=np.float64))
        its, rn = self.mg.cg(self._b, self._x, self.rtol, self.atol, self.max_it, full=self.hmg.full)
        out = self._x.get()
        if x is not None:
            x[:] = out
            out = x
        return out, its, rn

    def close(self):
        self.mg.close()


class DGMassInv(object):
    """The pressure-block preconditioner of the reference (alfi/solver.py:15-38), same PCPython protocol:
    ``y = -(nu + gamma) M_p^-1 x`` with the (diagonal, P0) pressure mass matrix.  ``pc.getAttr`` style context: the
    ``PC`` passed in must carry ``attrs["nu"], attrs["gamma"], attrs["mass_diag"]`` (the reference pulls nu and gamma
    from the application context, solver.py:17-21)."""

    def initialize(self, pc):
        self.update(pc)

    def update(self, pc):
        self.nu, self.gamma = float(pc.getAttr("nu")), float(pc.getAttr("gamma"))
        self.minv = 1.0 / np.asarray(pc.getAttr("mass_diag"), dtype=np.float64)

    def apply(self, pc, x, y):
        y[...] = -(self.nu + self.gamma) * self.minv * np.asarray(x)

    def matApply(self, pc, X, Y):
        """PCMatApply: ``apply`` on every column of the dense host matrix X into the same column of Y."""
        check_mat_apply_args(X, Y, len(self.minv))
        if isinstance(X, hip.DeviceMat) or isinstance(Y, hip.DeviceMat):
            raise ValueError("DGMassInv.matApply works on host matrices")
        _dense_array(Y)[...] = -(self.nu + self.gamma) * self.minv[:, None] * _dense_array(X)

    def applyTranspose(self, pc, x, y):
        raise NotImplementedError("Sorry!")


def outer_solver(tdim, fieldsplit_0, high_accuracy=False):
    """The ``outer`` dictionary of alfi/solver.py:402-499 for solver_type almg (Newton keys included verbatim; only the
    linear-solve keys are acted on by ``HipOuterSolver``)."""
    outer = {
        "snes_type": "newtonls", "snes_max_it": 20, "snes_linesearch_type": "basic", "snes_linesearch_maxstep": 1.0,
        "snes_monitor": None, "snes_linesearch_monitor": None, "snes_converged_reason": None,
        "ksp_type": "fgmres", "ksp_monitor_true_residual": None, "ksp_converged_reason": None,
        "mat_type": "nest", "ksp_max_it": 500,
        "pc_type": "fieldsplit", "pc_fieldsplit_type": "schur",
        "pc_fieldsplit_schur_factorization_type": "full", "pc_fieldsplit_schur_precondition": "user",
        "fieldsplit_0": fieldsplit_0,
        "fieldsplit_1": {"ksp_type": "preonly", "pc_type": "python", "pc_python_type": "alfi_amd.solver.DGMassInv"},
    }
    if high_accuracy:
        outer.update({"ksp_rtol": 1.0e-12, "ksp_atol": 1.0e-12})
    elif tdim == 2:
        outer.update({"ksp_rtol": 1.0e-9, "ksp_atol": 1.0e-10})
    else:
        outer.update({"ksp_rtol": 1.0e-8, "ksp_atol": 1.0e-8})
    return outer


class HipOuterSolver(object):
    """One linear solve of the reference's outer iteration (solver.py:386-422) on the GPU: KSPFGMRES (restart 30, the
    PETSc default the reference does not override) around PCFIELDSPLIT-Schur-full, fieldsplit_0 = the device PCMG
    (``HipMG``, ``fieldsplit_0_mg``) or the exact solve of the finest operator (``fieldsplit_0_lu``: multifrontal factors,
    only the finest level is uploaded), fieldsplit_1 = ``DGMassInv``.  ``solve(f, g)`` returns (u, p, iterations, true
    residual norm)."""

    def __init__(self, ctx, levels, transfers, params, restriction=False, coarse_inv=None, patch_factor_dtype=None):
        """patch_factor_dtype: HipMG's (None, or "f32": single-precision storage of the dense patch inverses where it exists)."""
        from .problem import build_pressure_coupling
        if params.get("ksp_type") != "fgmres" or params.get("pc_type") != "fieldsplit" \
                or params.get("pc_fieldsplit_type") != "schur" \
                or params.get("pc_fieldsplit_schur_factorization_type") != "full" \
                or params.get("pc_fieldsplit_schur_precondition") != "user":
            raise NotImplementedError("outer solver must be fgmres + fieldsplit schur/full/user (solver.py:402-411)")
        fs1 = params.get("fieldsplit_1", {})
        if fs1.get("ksp_type") != "preonly" or not str(fs1.get("pc_python_type", "")).endswith("DGMassInv"):
            raise NotImplementedError("fieldsplit_1 must be preonly + DGMassInv (solver.py:386-390)")
        self.ctx = ctx
        fs0 = params["fieldsplit_0"]
        self.direct = is_fieldsplit_0_lu(fs0)
        L = levels[-1]
        if self.direct:
            # the saddle solve needs the finest level only: a one-level hierarchy around it (no patches, no coarse inverse)
            self.hmg = None
            dl = hip.Level(ctx, L.A, L.bc_dofs)
            mg = hip.Multigrid.__new__(hip.Multigrid)
            hip.Multigrid._from_device_levels(mg, ctx, [dl], [], 1, False)
            self.mg = mg
        else:
            self.hmg = HipMG(ctx, levels, transfers, fs0, restriction=restriction, coarse_inv=coarse_inv,
                             patch_factor_dtype=patch_factor_dtype)
            if not self.hmg.full:
                raise NotImplementedError("fieldsplit_0 must use pc_mg_type full (solver.py:366)")
            self.mg = self.hmg.mg
        self.B, self.mass_diag = build_pressure_coupling(L)
        self.saddle = hip.Saddle(self.mg, self.B, self.mass_diag, L.nu, L.gamma, remove_constant_nullspace=True)
        if self.direct:
            self.saddle.set_velocity_solver("direct")
            self.saddle.factor_velocity()
        self.rtol, self.atol = float(params.get("ksp_rtol", 1e-5)), float(params.get("ksp_atol", 1e-50))
        self.max_it = int(params.get("ksp_max_it", 10000))
        self.restart = int(params.get("ksp_gmres_restart", 30))
        self.n_u, self.n_p = self.saddle.n_u, self.saddle.n_p

    def solve(self, f, g=None):
        b = np.concatenate([np.asarray(f, dtype=np.float64), np.zeros(self.n_p) if g is None else np.asarray(g)])
        db, dx = self.ctx.vec(b), self.ctx.vec(self.n_u + self.n_p)
        its, rn = self.saddle.solve(db, dx, self.rtol, self.atol, self.max_it, self.restart)
        x = dx.get()
        return x[:self.n_u], x[self.n_u:], its, rn
