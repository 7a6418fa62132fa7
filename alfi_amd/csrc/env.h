// Every environment switch of libalfi_hip.so, one accessor each: the ONLY file of csrc/ that calls getenv (tests/test_env_switches.py).
// The table in INTEGRATION.md lists the same names.  "once per process": parsed at the first call and kept; the others are
// parsed at every call, which their callers make at the time stated.  Host only.
#pragma once
#include <cstdint>
#include <cstdlib>

// ALFI_TEST_LARGE_PATHS (default 0; once per process) -- a TEST HOOK, not a tuning switch: 1 lowers to zero the size thresholds
// that select the kernels of the large levels (nnz-balanced SpMV with the fix-up launch and the de-duplicated x gathers instead
// of whole-row chunks, the general smoother chain instead of the fused iteration of small levels), so that the small hierarchies
// of the test suite run the code the 10 M-dof levels run.
inline bool alfi_test_large_paths() {
  static const bool on = getenv("ALFI_TEST_LARGE_PATHS") && atoi(getenv("ALFI_TEST_LARGE_PATHS")) == 1;
  return on;
}

// ALFI_MULT_PERSISTENT (default 1; once per process) -- 0: the multiplicative sweep as one launch per dependency wavefront (the
// schedule of rounds 1-3; kept for the bitwise comparison) instead of the persistent kernel.
inline bool alfi_env_mult_persistent() {
  static const bool on = !(getenv("ALFI_MULT_PERSISTENT") && atoi(getenv("ALFI_MULT_PERSISTENT")) == 0);
  return on;
}

// ALFI_INVERT_MFMA (default 1; once per process) -- 0: patches of 33 .. 160 dofs are inverted by the register kernel, never on
// the matrix cores; 2: the matrix-core kernel also takes the sizes up to 112 dofs, where the register kernel is faster (tests).
inline int alfi_env_invert_mfma() {
  static const int v = getenv("ALFI_INVERT_MFMA") ? atoi(getenv("ALFI_INVERT_MFMA")) : 1;
  return v;
}

// ALFI_PATCH_CHECK (default 1; once per process) -- 0: no residual probe (and no pivoted repair) of the patch inverses after a
// factorisation.
inline bool alfi_env_patch_check() {
  static const bool on = !(getenv("ALFI_PATCH_CHECK") && atoi(getenv("ALFI_PATCH_CHECK")) == 0);
  return on;
}

// ALFI_PATCH_CHECK_TOL (default 1e-6; once per process) -- probe residual above which a patch inverse is flagged and re-inverted
// with pivoting.
inline double alfi_env_patch_check_tol() {
  static const double v = getenv("ALFI_PATCH_CHECK_TOL") ? atof(getenv("ALFI_PATCH_CHECK_TOL")) : 1e-6;
  return v;
}

// ALFI_PATCH_CHECK_FAIL (default 1000 x the tolerance above; once per process) -- probe residual that still fails the set-up
// after the pivoted repair (below it a patch is ill-conditioned, not mis-factored: reported by alfi_patches_check, no error).
inline double alfi_env_patch_check_fail() {
  static const double v = getenv("ALFI_PATCH_CHECK_FAIL") ? atof(getenv("ALFI_PATCH_CHECK_FAIL")) : 1e3 * alfi_env_patch_check_tol();
  return v;
}

// ALFI_COARSE_CHECK_FAIL (default 1e-2; once per process) -- residual probe of the exact solves (coarse grid, allu) beyond which
// the set-up fails (round 2 failed at 1e-5: ADVICE r2 -- at Re 10 000 on fine coarse grids a merely ill-conditioned operator would
// have become a set-up error).
inline double alfi_env_coarse_check_fail() {
  static const double v = getenv("ALFI_COARSE_CHECK_FAIL") ? atof(getenv("ALFI_COARSE_CHECK_FAIL")) : 1e-2;
  return v;
}

// ALFI_BIG_SCRATCH_MB (default 6144; at every large-block factorisation) -- MiB of scratch (matrices + panels) per batch of patches.
inline int64_t alfi_env_big_scratch_bytes() {
  const char* e = getenv("ALFI_BIG_SCRATCH_MB");
  return e ? (int64_t)atoll(e) << 20 : (int64_t)6 << 30;
}

// ALFI_DIST_EXACT_NORM (default 1; at alfi_ctx_set_comm / alfi_ctx_comm_init) -- partitioned FGMRES: |w - V h| by an all-reduce of
// its own, as PETSc's VecNorm; 0: from |w|^2 - |h|^2 with the dots' all-reduce (one reduction fewer per iteration; absolute error
// eps |w|^2, so a new direction that is small against w is mis-normalised -- measurements only).
inline bool alfi_env_dist_exact_norm() {
  const char* e = getenv("ALFI_DIST_EXACT_NORM");
  return !(e && atoi(e) == 0);
}

// ALFI_RCCL_LIB (default unset; when librccl is loaded, at the first alfi_ctx_comm_init) -- a library tried before librccl.so.1,
// librccl.so and the ROCm install's copy (the test suite's shared-memory stand-in); NULL when unset.
inline const char* alfi_env_rccl_lib() { return getenv("ALFI_RCCL_LIB"); }

// NOT an environment switch (and on purpose not tied to the test hook at the top of this file: the small hierarchies of the
// test suite keep their dense inverses) -- the default of alfi_ctx_set_condense_min_bytes, kept with the other defaults: a level
// without caller-supplied groups whose dense patch inverses would take at least this many bytes looks for condensable groups
// when it factors.  1 GiB: config 4's two large levels (3.8 and 31.9 GB) condense; its 0.44 GB level, 729-patch launches that
// are launch-bound either way, keeps the one-launch dense apply (three launches per apply would cost it 2 x 20 launches a cycle).
inline int64_t alfi_default_condense_min_bytes() { return (int64_t)1 << 30; }
