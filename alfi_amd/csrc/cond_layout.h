// Layout of the condensed patch factors that the host planner (patch_plan.h) and the kernels (kernels_bigpatch.hip) share: the
// chunk descriptor and the storage of one group's matrices.  Plain C++ for a host compiler, __host__ __device__ under hipcc.
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define ALFI_HD __host__ __device__
#else
#define ALFI_HD
#endif

// a chunk of consecutive groups of one patch (<= COND_CHUNK_PAIRS row pairs of X / W and of B): the work unit of cond_gfront /
// cond_gback, one descriptor per workgroup
struct CondChunk {
  int64_t off;        // patch_ptr[p]
  int64_t ubase;      // uptr[p]
  int64_t sidx0;      // first entry of the chunk's S_g lists in CondDev::sidx
  int64_t stage_off;  // stage_ptr[p]
  int32_t xq0, xq1;   // the chunk's X / W row pairs in xpd
  int32_t bq0, bq1;   // the chunk's B row pairs in bpd
  int32_t e0, ne;     // its interior entries (adjacent in the condensed order)
  int32_t u0, nu;     // its entries of the patch's u layout
  int32_t nI;
  int32_t xp0, bp0;   // first row pair of the PATCH in the X / W and in the B numbering (a pair's place inside its group)
  int32_t pad;
};

// rows of inv(Sigma) per workgroup of the sigma kernels of the condensed apply (4 waves; kernels_bigpatch.hip, chunk table in
// plan_condensed)
#ifndef ALFI_COND_SIGMA_ROWS
#define ALFI_COND_SIGMA_ROWS 64
#endif
constexpr int COND_SIGMA_ROWS = ALFI_COND_SIGMA_ROWS;

// Launches of at least this many patches take the workgroup-per-patch form of the condensed apply (cond_front / cond_sigma /
// cond_back), smaller ones the chunked form (launch_cond_apply_range, kernels_bigpatch.hip).  The block apply batches the
// workgroup-per-patch form alone (kernels_block_cond.hip).
constexpr int64_t COND_PER_PATCH_MIN = 1024;

// Waves per patch of the workgroup-per-patch form: a lane owns one row pair per phase, so a workgroup wider than the patch's
// row pairs (max_pairs: most row pairs of X / W or of B in one patch of the level) is idle lanes.
ALFI_HD inline int cond_patch_waves(int max_pairs) {
#ifdef ALFI_COND_WAVES_FORCE      // A/B builds only (scripts/build_variant.sh): every launch with this many waves per patch
  (void)max_pairs;
  return ALFI_COND_WAVES_FORCE;
#else
  return max_pairs <= 64 ? 1 : max_pairs <= 128 ? 2 : max_pairs <= 256 ? 4 : 8;
#endif
}

// The early-load form of cond_front_kernel (kernels_bigpatch.hip): a lane requests its tables and ALL columns of its row pair
// of X or of B at kernel entry, ahead of the barriers they do not depend on.  A level takes it when a group's matrix fits one
// batch of COND_AHEAD_M 16-byte loads per lane and every phase of every patch is one pass (a lane owns at most one row pair of
// X / W and one of B).  Macro stars (groups of 45, thousands of pairs) keep the loops.
#ifndef ALFI_COND_AHEAD           // A/B builds only (scripts/build_variant.sh): 0 compiles the dispatch without the early-load form
#define ALFI_COND_AHEAD 1
#endif
constexpr int COND_AHEAD_M = 16;
ALFI_HD inline bool cond_ahead(int max_m, int max_pairs) {
  return ALFI_COND_AHEAD != 0 && max_m <= COND_AHEAD_M && max_pairs <= 64 * cond_patch_waves(max_pairs);
}
// Waves per patch of the early-load front kernel: the X pairs and the B pairs of a patch go to DIFFERENT waves (a wave holds one
// matrix batch in registers, not two), whole waves each.
ALFI_HD inline int cond_ahead_front_waves(int xpairs, int bpairs) { return (xpairs + 63) / 64 + (bpairs + 63) / 64; }

// The tail launch of the workgroup-per-patch form (cond_tail_kernel, kernels_bigpatch.hip): y_S = inv(Sigma) rhs and the back
// substitution of a patch in ONE workgroup of 256 threads, y_S through LDS.  A row pair of W belongs to four adjacent lanes, a
// quarter of COND_TAIL_QUARTER columns each, all requested at kernel entry with the wave's block of inv(Sigma).  A level takes
// it when every patch has a lane quartet per row pair of X / W (max_xpairs), every group's W fits the four quarters (max_sc:
// most coupled skeleton entries of one group) and every skeleton is one chunk of the sigma launch (max_s).  Macro stars
// (hundreds of pairs, skeletons of hundreds of rows) keep cond_sigma + cond_back.
#ifndef ALFI_COND_TAIL            // A/B builds only (scripts/build_variant.sh): 0 compiles the dispatch without the tail launch
#define ALFI_COND_TAIL 1
#endif
constexpr int COND_TAIL_THREADS = 256;
constexpr int COND_TAIL_QUARTER = 8;      // (= COND_U, cond_apply.h: one batch of 16-byte loads per lane)
constexpr int COND_TAIL_S = 64;           // 16 rows of inv(Sigma) per wave, held whole in one batch of loads
ALFI_HD inline bool cond_tail(int max_xpairs, int max_sc, int max_s) {
  return ALFI_COND_TAIL != 0 && 4 * max_xpairs <= COND_TAIL_THREADS && max_sc <= 4 * COND_TAIL_QUARTER &&
         max_s <= COND_SIGMA_ROWS && max_s <= COND_TAIL_S;
}

// storage of one group's matrices in CondDev::mat: [X (m x m) | B (sc x m) | W (m x sc)], column-major each, the leading
// dimensions rounded up to EVEN (a lane streams two rows of a column with one 16-byte load; the pad row is never stored)
// (Measured and dropped, round 5: leading dimensions of > 8 rows rounded up to whole 128-byte lines and every group on a line
// boundary -- no column shares a line with its neighbour, +3.8 % bytes: config 5 24.13 against 23.60-23.68 ms per cycle, same box.)
ALFI_HD inline int cond_ldim(int rows) { return (rows + 1) & ~1; }
ALFI_HD inline int cond_pairs(int rows) { return (rows + 1) / 2; }     // row pairs a lane each
ALFI_HD inline int64_t cond_group_doubles(int m, int sc) {
  return (int64_t)cond_ldim(m) * m + (int64_t)cond_ldim(sc) * m + (int64_t)cond_ldim(m) * sc;
}
