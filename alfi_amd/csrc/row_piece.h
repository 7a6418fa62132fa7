// The hot loop of every apply that streams a stored dense inverse (kernels_patch.hip: additive apply in both storage precisions,
// the sweep of a workgroup per small patch; kernels_bigpatch.hip: macro stars in both precisions, their sweep, the inverse of a
// condensed level's Schur complement), written once.
//
// Storage (piece_index, patch_plan.h): the rows of an n x n inverse, padded to ld = n rounded up to V, are cut into row pieces
// of 128 rows and then the binary digits of the remainder down to V; a piece of R rows is stored [column][R].  G = R / V lanes
// share a column -- lane l holds rows V l .. V l + V - 1 as ONE aligned 16-byte load --, so a wave instruction covers C = 64 / G
// columns = 1 KiB of consecutive bytes.  Two parameterisations (RowPiece<S>):
//     S = double: V = 2 rows per lane, pieces 128 .. 2        S = float: V = 4 rows per lane, pieces 128 .. 4
// Every product and every sum is FP64 whatever S: __builtin_fma((double)v, x, acc).
//
// Summation order of a row (what the bitwise tests pin: split launches = full launches, partitioned levels = serial ones,
// tests/test_gpu_row_piece_bits.py): ascending columns cg, cg + C, ... inside a lane, then the column groups by
// acc += __shfl_xor(acc, o) for o = G, 2 G, ..., 32.  U and the tail policy change which loads are in flight together, never
// the order of the sums.
//
// TWO bodies implement this order and must be kept in step: piece_dot / piece_apply for one vector (what every single-vector
// kernel is compiled from) and their NV forms for 2 .. 4 vectors per stream (block right-hand sides, kernels_block.hip), whose
// per-vector products and sums are the one-vector ones.  One template for both was tried three ways -- NV = 1 forwarded to the NV
// body, `if constexpr (NV == 1)` around its stores, a shared per-value helper: each compiled the single-vector kernels of
// kernels_bigpatch.hip or kernels_patch.hip to other code (scripts/device_code_equal.py), so the one-vector bodies stay verbatim.
// tests/test_gpu_block_rhs.py compares the two bit for bit at every piece width.
#pragma once
#include <type_traits>
#include "patch_plan.h"

template <typename S>
struct RowPiece;
template <>
struct RowPiece<double> {
  static constexpr int V = 2;                                 // rows of a column per lane
  typedef double vec __attribute__((ext_vector_type(2)));     // ... as one 16-byte load
  ALFI_HD static int ld(int n) { return (n + 1) & ~1; }
};
template <>
struct RowPiece<float> {
  static constexpr int V = F32_ROWS;
  typedef float vec __attribute__((ext_vector_type(F32_ROWS)));
  ALFI_HD static int ld(int n) { return f32_ld(n); }
};

#ifdef __HIPCC__
// a lane's V rows of one column: one aligned 16-byte load
template <typename S, bool NT>
__device__ __forceinline__ typename RowPiece<S>::vec piece_load(const S* p) {
  const typename RowPiece<S>::vec* q = reinterpret_cast<const typename RowPiece<S>::vec*>(p);
  return NT ? __builtin_nontemporal_load(q) : *q;
}

// acc[k] = sum over the columns j = cg, cg + C, ... < n of (double)base[j * stride + k] * xs[j], summed over the column groups.
// base: the lane's V rows of column 0; stride: elements from one column to the next (V G for a whole piece).
// U loads are in flight per lane.  BATCH_TAIL: the last, partial group of U columns is requested together too (levels of many
// small patches); otherwise the tail is a column at a time (macro stars: the tail is a small share of n columns).
template <typename S, int G, bool NT, int U, bool BATCH_TAIL>
__device__ __forceinline__ void piece_dot(const S* __restrict__ base, int stride, int n, const double* __restrict__ xs, int cg,
                                          double (&acc)[RowPiece<S>::V]) {
  typedef typename RowPiece<S>::vec vec;
  constexpr int C = 64 / G, V = RowPiece<S>::V;
#pragma unroll
  for (int k = 0; k < V; ++k) acc[k] = 0.0;
  int j = cg;
  for (; j + (U - 1) * C < n; j += U * C) {
    vec v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = piece_load<S, NT>(base + (int64_t)(j + u * C) * stride);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const double xj = xs[j + u * C];
#pragma unroll
      for (int k = 0; k < V; ++k) acc[k] = __builtin_fma((double)v[u][k], xj, acc[k]);
    }
  }
  if constexpr (BATCH_TAIL) {
    if (j < n) {
      const vec zero = {};
      vec v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) v[u] = j + u * C < n ? piece_load<S, NT>(base + (int64_t)(j + u * C) * stride) : zero;
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (j + u * C < n) {
          const double xj = xs[j + u * C];
#pragma unroll
          for (int k = 0; k < V; ++k) acc[k] = __builtin_fma((double)v[u][k], xj, acc[k]);
        }
    }
  } else {
    for (; j < n; j += C) {
      const vec v = piece_load<S, NT>(base + (int64_t)j * stride);
      const double xj = xs[j];
#pragma unroll
      for (int k = 0; k < V; ++k) acc[k] = __builtin_fma((double)v[k], xj, acc[k]);
    }
  }
  if (C > 1) {
#pragma unroll
    for (int o = G; o < 64; o <<= 1) {
#pragma unroll
      for (int k = 0; k < V; ++k) acc[k] += __shfl_xor(acc[k], o);
    }
  }
}

// What the first column group does with its V sums: PAIR -- one unconditional 16-byte store (S = double; the pad row of the
// inverse is zero and ``out`` has ld slots); ALL -- V unconditional scalars (``out`` has RowPiece<S>::ld(n) slots); GUARDED -- the
// rows below ``lim`` only (``out`` ends with the last row that exists: a pad row's sum is never written).
enum class PieceStore { PAIR, ALL, GUARDED };

// One block of V G rows of a stored piece times xs[0 .. n): T points at (first row of the block, column 0).  lim: the rows of
// the block that exist (read by GUARDED alone; the other stores pass 0).
template <typename S, int G, bool NT, int U, bool BATCH_TAIL, PieceStore ST>
__device__ __forceinline__ void piece_apply(const S* __restrict__ T, int stride, int n, const double* __restrict__ xs, int lane,
                                            double* __restrict__ out, int lim) {
  constexpr int V = RowPiece<S>::V;
  const int cg = lane / G, l = lane % G;
  double acc[V];
  piece_dot<S, G, NT, U, BATCH_TAIL>(T + V * l, stride, n, xs, cg, acc);
  if (cg != 0) return;
  if constexpr (ST == PieceStore::PAIR) {
    static_assert(V == 2, "a row pair");
    *reinterpret_cast<double2*>(out + 2 * l) = make_double2(acc[0], acc[1]);
  } else {
#pragma unroll
    for (int k = 0; k < V; ++k)
      if (ST == PieceStore::ALL || V * l + k < lim) out[V * l + k] = acc[k];
  }
}

// ---- block right-hand sides: the same for NV = 2 .. 4 vectors per stream of the stored values -----------------------------------
// acc[c][k] = sum over the columns j of (double)base[j * stride + k] * xs[j * NV + c]: every stored value is loaded ONCE and
// multiplied into NV accumulators; the products and sums of right-hand side c are exactly those of piece_dot above on that
// vector, in the order stated at the top (column c of a block apply is the single apply bit for bit).  xs: the NV gathered
// vectors interleaved entry by entry, so that the NV values of a column are consecutive in LDS.
// (A template of its own, not piece_dot with NV = 1 forwarded to it: the forwarded form compiles the macro stars' kernels to
// other register allocations -- scripts/device_code_equal.py --, and the single-vector kernels are to stay what they were.)
template <typename S, int G, bool NT, int U, bool BATCH_TAIL, int NV>
__device__ __forceinline__ void piece_dot(const S* __restrict__ base, int stride, int n, const double* __restrict__ xs, int cg,
                                          double (&acc)[NV][RowPiece<S>::V]) {
  typedef typename RowPiece<S>::vec vec;
  constexpr int C = 64 / G, V = RowPiece<S>::V;
  static_assert(NV >= 1 && NV <= 4, "one to four right-hand sides per stream of the stored values");
  auto fma_all = [&](const vec& v, int j) {      // the NV accumulators take one loaded value each
#pragma unroll
    for (int c = 0; c < NV; ++c) {
      const double xj = xs[j * NV + c];
#pragma unroll
      for (int k = 0; k < V; ++k) acc[c][k] = __builtin_fma((double)v[k], xj, acc[c][k]);
    }
  };
#pragma unroll
  for (int c = 0; c < NV; ++c)
#pragma unroll
    for (int k = 0; k < V; ++k) acc[c][k] = 0.0;
  int j = cg;
  for (; j + (U - 1) * C < n; j += U * C) {
    vec v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = piece_load<S, NT>(base + (int64_t)(j + u * C) * stride);
#pragma unroll
    for (int u = 0; u < U; ++u) fma_all(v[u], j + u * C);
  }
  if constexpr (BATCH_TAIL) {
    if (j < n) {
      const vec zero = {};
      vec v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) v[u] = j + u * C < n ? piece_load<S, NT>(base + (int64_t)(j + u * C) * stride) : zero;
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (j + u * C < n) fma_all(v[u], j + u * C);
    }
  } else {
    for (; j < n; j += C) fma_all(piece_load<S, NT>(base + (int64_t)j * stride), j);
  }
  if (C > 1) {
#pragma unroll
    for (int o = G; o < 64; o <<= 1) {
#pragma unroll
      for (int c = 0; c < NV; ++c)
#pragma unroll
        for (int k = 0; k < V; ++k) acc[c][k] += __shfl_xor(acc[c][k], o);
    }
  }
}

// piece_apply for NV vectors: the sums of right-hand side c go to out + c * ostride
template <typename S, int G, bool NT, int U, bool BATCH_TAIL, PieceStore ST, int NV>
__device__ __forceinline__ void piece_apply(const S* __restrict__ T, int stride, int n, const double* __restrict__ xs, int lane,
                                            double* __restrict__ out, int ostride, int lim) {
  constexpr int V = RowPiece<S>::V;
  const int cg = lane / G, l = lane % G;
  double acc[NV][V];
  piece_dot<S, G, NT, U, BATCH_TAIL, NV>(T + V * l, stride, n, xs, cg, acc);
  if (cg != 0) return;
#pragma unroll
  for (int c = 0; c < NV; ++c) {
    double* o = out + c * ostride;
    if constexpr (ST == PieceStore::PAIR) {
      static_assert(V == 2, "a row pair");
      *reinterpret_cast<double2*>(o + 2 * l) = make_double2(acc[c][0], acc[c][1]);
    } else {
#pragma unroll
      for (int k = 0; k < V; ++k)
        if (ST == PieceStore::ALL || V * l + k < lim) o[V * l + k] = acc[c][k];
    }
  }
}

// The pieces of ld stored rows (a multiple of MIN_ROWS) in storage order: f(integral_constant<int, R>, row0, piece_no) for the
// 128-row pieces and then for every set binary digit R >= MIN_ROWS of the remainder.
// (The callers' lambdas capture by value: by reference the FP32 apply of small patches takes two more VGPRs.  mult_wg_apply,
// kernels_patch.hip, keeps its walk written out for the same reason.)
template <int R, int MIN_ROWS, typename F>
__device__ __forceinline__ void walk_digits(int rem, int& row0, int& piece, F& f) {
  if constexpr (R >= MIN_ROWS) {
    if (rem & R) {
      f(std::integral_constant<int, R>{}, row0, piece);
      row0 += R;
      ++piece;
    }
    walk_digits<R / 2, MIN_ROWS>(rem, row0, piece, f);
  }
}
template <int MIN_ROWS, typename F>
__device__ __forceinline__ void walk_pieces(int ld, F f) {
  int row0 = 0, piece = 0;
  for (; row0 + 128 <= ld; row0 += 128, ++piece) f(std::integral_constant<int, 128>{}, row0, piece);
  walk_digits<64, MIN_ROWS>(ld - row0, row0, piece, f);
}
#endif
