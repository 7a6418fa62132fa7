// Device helpers of the condensed apply that its one-vector kernels (kernels_bigpatch.hip) and its block forms
// (kernels_block_cond.hip) share: the walk over the stored row pieces of inv(Sigma) in aligned power-of-two blocks (big_block,
// big_rows, and a block in two halves: big_block_prefetch / big_block_finish) and the row-pair product of the group matrices
// (cond_wave_max, cond_row2_dot).  The one-vector bodies are what every single-vector kernel is compiled from; the NV forms
// below them (2 .. 4 right-hand sides per stream of the stored values) hold the per-vector state NV times: per right-hand side
// the same products and the same sums in the same order (row_piece.h records why the two are separate bodies).
#pragma once
#include "row_piece.h"

#ifdef __HIPCC__
typedef double big_d2 __attribute__((ext_vector_type(2)));
constexpr int BIG_U = 8;            // 16-byte loads in flight per lane (piece_dot, row_piece.h); the tail a column at a time

// Rows [r0, r1) of y = T x for a wave, T in the row-piece layout (pieces of 128 rows, then the binary digits of the rest;
// piece (row0, P rows): entry (r, c) at T[row0 * n + c * P + (r - row0)]).  The range is cut into aligned power-of-two
// blocks of rows inside the stored pieces: a block of 2 G rows takes G lanes per column and 64 / G columns per load
// instruction.  Used where whole pieces dealt round-robin leave waves idle (a Schur complement of 312 rows is
// 2 x 128 + 32 + 16 + 8: two of eight waves would stream 82 % of it).
// the next block of a range of rows [r, r1): the stored piece (row0, P rows) that holds row r and R, the rows of the block
__device__ __forceinline__ void big_block(int ld, int r, int r1, int& row0, int& P, int& R) {
  const int full = ld & ~127;
  if (r < full) {
    row0 = r & ~127;
    P = 128;
  } else {
    row0 = full;
    P = 64;
    const int rem = ld - full;
    for (; P >= 2; P >>= 1)
      if (rem & P) {
        if (r < row0 + P) break;
        row0 += P;
      }
  }
  const int o = r - row0;
  R = P;                               // the largest aligned power-of-two block at o that ends inside the piece and the range
  while (R > 2 && ((o & (R - 1)) != 0 || o + R > P || r + R > r1)) R >>= 1;
}

template <bool NT>
__device__ __forceinline__ void big_rows(const double* __restrict__ T, int n, int ld, int r0, int r1,
                                         const double* __restrict__ xs, int lane, double* __restrict__ ys) {
  // ys: n doubles (LDS or global); rows >= n (the zero pad row) are not stored
  int r = r0;
  while (r < r1) {
    int row0, P, R;
    big_block(ld, r, r1, row0, P, R);
    const int o = r - row0;
    const double* Tp = T + (int64_t)row0 * n + o;
    // (lim = n - r: the pad row of an odd n is not written)
#define ALFI_BIG_BLOCK(RV) \
  case RV: piece_apply<double, RV / 2, NT, BIG_U, false, PieceStore::GUARDED>(Tp, P, n, xs, lane, ys + r, n - r); break;
    switch (R) {
      ALFI_BIG_BLOCK(128) ALFI_BIG_BLOCK(64) ALFI_BIG_BLOCK(32) ALFI_BIG_BLOCK(16) ALFI_BIG_BLOCK(8) ALFI_BIG_BLOCK(4)
      default: piece_apply<double, 1, NT, BIG_U, false, PieceStore::GUARDED>(Tp, P, n, xs, lane, ys + r, n - r); break;
    }
#undef ALFI_BIG_BLOCK
    r += R;
  }
}

// One block of big_rows in two halves, for a kernel that requests the block before its operand exists: the loads of a block of
// R = 2 << lg <= 16 rows over n <= BIG_U * 64 / (R / 2) columns -- every column group of the lane, BIG_U 16-byte loads held in
// registers -- and, later, the sums.  The sums are those of piece_apply<double, R / 2, ., BIG_U, false, GUARDED> to the bit: a
// lane's columns ascending, then the column groups by shuffles (row_piece.h).  Tp: (first row of the block, column 0), P: the
// rows of the stored piece.
template <bool NT>
__device__ __forceinline__ void big_block_prefetch(const double* __restrict__ Tp, int P, int n, int lg, int lane,
                                                   big_d2 (&v)[BIG_U]) {
  const int C = 64 >> lg, cg = lane >> lg, l = lane & ((1 << lg) - 1);
#pragma unroll
  for (int u = 0; u < BIG_U; ++u) {
    const big_d2 z = {0.0, 0.0};
    v[u] = cg + u * C < n ? piece_load<double, NT>(Tp + 2 * l + (int64_t)(cg + u * C) * P) : z;
  }
}
__device__ __forceinline__ void big_block_finish(const big_d2 (&v)[BIG_U], int n, int lg, const double* __restrict__ xs, int lane,
                                                 double* __restrict__ out, int lim) {
  const int G = 1 << lg, C = 64 >> lg, cg = lane >> lg, l = lane & (G - 1);
  double acc0 = 0.0, acc1 = 0.0;
#pragma unroll
  for (int u = 0; u < BIG_U; ++u)
    if (cg + u * C < n) {
      const double xj = xs[cg + u * C];
      acc0 = __builtin_fma(v[u].x, xj, acc0);
      acc1 = __builtin_fma(v[u].y, xj, acc1);
    }
  for (int o = G; o < 64; o <<= 1) {
    acc0 += __shfl_xor(acc0, o);
    acc1 += __shfl_xor(acc1, o);
  }
  if (cg != 0) return;
  if (2 * l < lim) out[2 * l] = acc0;
  if (2 * l + 1 < lim) out[2 * l + 1] = acc1;
}

// The same two halves for a kernel that holds SEVERAL small blocks of a wave's rows in one array of BIG_U loads
// (cond_tail_kernel, kernels_bigpatch.hip: blocks of 8, 4 and 2 rows over <= 64 columns are 4 + 2 + 1 loads).  A block whose
// columns fit U <= BIG_U loads per lane, n <= U * 64 / (R / 2): the loads into v[0 .. U), the sums those of big_block_finish
// (the loads it would skip are not there).  u0: the request is for the loads u0 .. u0 + U - 1 of big_block_prefetch (a block
// requested in several calls).
template <bool NT, int U>
__device__ __forceinline__ void big_part_prefetch(const double* __restrict__ Tp, int P, int n, int lg, int lane, int u0,
                                                  big_d2* v) {
  const int C = 64 >> lg, cg = lane >> lg, l = lane & ((1 << lg) - 1);
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const big_d2 z = {0.0, 0.0};
    v[u] = cg + (u0 + u) * C < n ? piece_load<double, NT>(Tp + 2 * l + (int64_t)(cg + (u0 + u) * C) * P) : z;
  }
}
template <int U>
__device__ __forceinline__ void big_part_finish(const big_d2* v, int n, int lg, const double* __restrict__ xs, int lane,
                                                 double* __restrict__ out, int lim) {
  const int G = 1 << lg, C = 64 >> lg, cg = lane >> lg, l = lane & (G - 1);
  double acc0 = 0.0, acc1 = 0.0;
#pragma unroll
  for (int u = 0; u < U; ++u)
    if (cg + u * C < n) {
      const double xj = xs[cg + u * C];
      acc0 = __builtin_fma(v[u].x, xj, acc0);
      acc1 = __builtin_fma(v[u].y, xj, acc1);
    }
  for (int o = G; o < 64; o <<= 1) {
    acc0 += __shfl_xor(acc0, o);
    acc1 += __shfl_xor(acc1, o);
  }
  if (cg != 0) return;
  if (2 * l < lim) out[2 * l] = acc0;
  if (2 * l + 1 < lim) out[2 * l + 1] = acc1;
}

// The small matrices of a group are streamed with COND_U loads in flight per lane (they are read once).
constexpr int COND_U = 8;

// wave-wide maximum of a small non-negative int
__device__ __forceinline__ int cond_wave_max(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
  return v;
}

// TWO ROWS of a group product per lane (rows 2 i, 2 i + 1 of a column-major block with an even leading dimension: one
// 16-byte load per column):   acc += sum_{k < kn} M[k * ld + (0, 1)] * v[k],   M -> the lane's rows, v -> LDS (the group's
// operand).  kn differs between the lanes of a wave; the loop runs to the wave's maximum with the loads predicated.
template <bool NT, int RU>
__device__ __forceinline__ void cond_row2_dot(const double* __restrict__ M, int ld, int kn, const double* __restrict__ v,
                                              double& acc0, double& acc1) {
  const int kmax = cond_wave_max(kn);
  for (int k = 0; k < kmax; k += RU) {
    big_d2 a[RU];
#pragma unroll
    for (int u = 0; u < RU; ++u) {
      const big_d2* q = reinterpret_cast<const big_d2*>(M + (int64_t)(k + u) * ld);
      const big_d2 z = {0.0, 0.0};
      a[u] = (k + u < kn) ? (NT ? __builtin_nontemporal_load(q) : *q) : z;
    }
#pragma unroll
    for (int u = 0; u < RU; ++u) {
      const double vk = (k + u < kn) ? v[k + u] : 0.0;
      acc0 = __builtin_fma(a[u].x, vk, acc0);
      acc1 = __builtin_fma(a[u].y, vk, acc1);
    }
  }
}

// ---- block right-hand sides: the same for NV = 2 .. 4 vectors per stream of the stored values --------------------------------
// Operands in LDS are interleaved entry by entry, v[i * NV + c] (piece_dot, row_piece.h); the sums of right-hand side c go to
// out + c * ostride.
template <bool NT, int NV>
__device__ __forceinline__ void big_rows(const double* __restrict__ T, int n, int ld, int r0, int r1,
                                         const double* __restrict__ xs, int lane, double* __restrict__ ys, int64_t ostride) {
  int r = r0;
  while (r < r1) {
    int row0, P, R;
    big_block(ld, r, r1, row0, P, R);
    const int o = r - row0;
    const double* Tp = T + (int64_t)row0 * n + o;
#define ALFI_BIG_BLOCK(RV)                                                                                                  \
  case RV:                                                                                                                  \
    piece_apply<double, RV / 2, NT, BIG_U, false, PieceStore::GUARDED, NV>(Tp, P, n, xs, lane, ys + r, ostride, n - r);      \
    break;
    switch (R) {
      ALFI_BIG_BLOCK(128) ALFI_BIG_BLOCK(64) ALFI_BIG_BLOCK(32) ALFI_BIG_BLOCK(16) ALFI_BIG_BLOCK(8) ALFI_BIG_BLOCK(4)
      default: piece_apply<double, 1, NT, BIG_U, false, PieceStore::GUARDED, NV>(Tp, P, n, xs, lane, ys + r, ostride, n - r); break;
    }
#undef ALFI_BIG_BLOCK
    r += R;
  }
}

// (the loads of a block are those of big_block_prefetch whatever NV)
template <int NV>
__device__ __forceinline__ void big_block_finish(const big_d2 (&v)[BIG_U], int n, int lg, const double* __restrict__ xs, int lane,
                                                 double* __restrict__ out, int64_t ostride, int lim) {
  const int G = 1 << lg, C = 64 >> lg, cg = lane >> lg, l = lane & (G - 1);
  double acc[NV][2];
#pragma unroll
  for (int c = 0; c < NV; ++c) acc[c][0] = acc[c][1] = 0.0;
#pragma unroll
  for (int u = 0; u < BIG_U; ++u)
    if (cg + u * C < n) {
#pragma unroll
      for (int c = 0; c < NV; ++c) {
        const double xj = xs[(cg + u * C) * NV + c];
        acc[c][0] = __builtin_fma(v[u].x, xj, acc[c][0]);
        acc[c][1] = __builtin_fma(v[u].y, xj, acc[c][1]);
      }
    }
  for (int o = G; o < 64; o <<= 1) {
#pragma unroll
    for (int c = 0; c < NV; ++c) {
      acc[c][0] += __shfl_xor(acc[c][0], o);
      acc[c][1] += __shfl_xor(acc[c][1], o);
    }
  }
  if (cg != 0) return;
#pragma unroll
  for (int c = 0; c < NV; ++c) {
    if (2 * l < lim) out[c * ostride + 2 * l] = acc[c][0];
    if (2 * l + 1 < lim) out[c * ostride + 2 * l + 1] = acc[c][1];
  }
}

// cond_row2_dot for NV operands: one 16-byte load per column, NV x 2 fma; the loop bound is the wave maximum of kn, loads and
// operands predicated as above (the zero-padded products are part of every sum, as they are in the one-vector body)
template <bool NT, int RU, int NV>
__device__ __forceinline__ void cond_row2_dot(const double* __restrict__ M, int ld, int kn, const double* __restrict__ v,
                                              double (&acc)[NV][2]) {
  const int kmax = cond_wave_max(kn);
  for (int k = 0; k < kmax; k += RU) {
    big_d2 a[RU];
#pragma unroll
    for (int u = 0; u < RU; ++u) {
      const big_d2* q = reinterpret_cast<const big_d2*>(M + (int64_t)(k + u) * ld);
      const big_d2 z = {0.0, 0.0};
      a[u] = (k + u < kn) ? (NT ? __builtin_nontemporal_load(q) : *q) : z;
    }
#pragma unroll
    for (int u = 0; u < RU; ++u) {
#pragma unroll
      for (int c = 0; c < NV; ++c) {
        const double vk = (k + u < kn) ? v[(k + u) * NV + c] : 0.0;
        acc[c][0] = __builtin_fma(a[u].x, vk, acc[c][0]);
        acc[c][1] = __builtin_fma(a[u].y, vk, acc[c][1]);
      }
    }
  }
}
#endif
