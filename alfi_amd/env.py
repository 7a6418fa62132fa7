"""Every ``ALFI_*`` environment switch the package reads, one function each: the ONLY module of alfi_amd that looks into
``os.environ`` for them (tests/test_env_switches.py).  The table in INTEGRATION.md lists the same names, with the switches
libalfi_hip.so reads itself (csrc/env.h).  Each function reads the environment when it is called; "read" below says when the
package calls it.  Standard library only: ``import alfi_amd.dist`` stays free of torch and of the native library.
"""
import os


def hip_lib():
    """ALFI_HIP_LIB (default unset -> None: alfi_amd/libalfi_hip.so): path of another build of the library (kernel tuning
    experiments, scripts/build_variant.sh).  Read once, when alfi_amd._lib is imported."""
    return os.environ.get("ALFI_HIP_LIB") or None


def host_threads():
    """ALFI_HOST_THREADS (default 0 = the process's share of the cores): threads of the host generator libalfi_host.so; overrides
    OMP_NUM_THREADS (torch.distributed.run exports OMP_NUM_THREADS=1 to every rank).  Read once, when that library is loaded."""
    return int(os.environ.get("ALFI_HOST_THREADS", "0"))


def condense():
    """ALFI_CONDENSE (default on; off only with "0"): macro-star patch factors are stored condensed where the level allows it.
    Read whenever a level's patches are set up (hip.condense_patches, solver.HipPatchPC)."""
    return os.environ.get("ALFI_CONDENSE", "1") != "0"


def coarse_sparse_min():
    """ALFI_COARSE_SPARSE_MIN (default 8192): coarse grids from this many dofs on get the sparse factorisation when the mode
    is "auto".  Read at every coarse factorisation in that mode."""
    return int(os.environ.get("ALFI_COARSE_SPARSE_MIN", 8192))


def device_assembly():
    """ALFI_DEVICE_ASSEMBLY (default on; off only with "0"): the Newton solvers refresh their operators on the device.  Read
    when a solver is constructed without an explicit ``device_assembly``."""
    return os.environ.get("ALFI_DEVICE_ASSEMBLY", "1") != "0"


def macrostar_literal():
    """ALFI_MACROSTAR_LITERAL (default off; on only with "1"): MacroStar patches by the constructor's own point-by-point walk
    instead of the incidence products.  Read whenever the patches of a Scott-Vogelius level are built."""
    return os.environ.get("ALFI_MACROSTAR_LITERAL") == "1"


def dist_transport():
    """ALFI_DIST_TRANSPORT (default unset -> None: "rccl" on an nccl process group, else "callback"): transport of the exchange
    points of partitioned levels.  Read when a DistMultigrid is constructed without ``transport``."""
    return os.environ.get("ALFI_DIST_TRANSPORT") or None


def dist_overlap():
    """ALFI_DIST_OVERLAP (default on; off only with "0"): halo exchanges overlap with interior work.  Read when a DistMultigrid
    is constructed without ``overlap``."""
    return os.environ.get("ALFI_DIST_OVERLAP", "1") != "0"


def dist_overlap_min_dofs():
    """ALFI_DIST_OVERLAP_MIN_DOFS (default unset -> None: the overlap rule decides per level): smallest per-rank share of a
    level that overlaps (tests, measurements).  Read when a DistMultigrid is constructed without ``overlap_min_dofs``."""
    return int(os.environ["ALFI_DIST_OVERLAP_MIN_DOFS"]) if "ALFI_DIST_OVERLAP_MIN_DOFS" in os.environ else None


def dist_global_generation():
    """ALFI_DIST_GLOBAL_GENERATION (default off; on only with "1"): the partitioned Newton solver generates the global hierarchy
    on every rank instead of rank-local pieces.  Read when the solver decides how to generate (at construction)."""
    return os.environ.get("ALFI_DIST_GLOBAL_GENERATION") == "1"
