// Device helpers of the two-stage reductions and of the paired BLAS-1 loads, shared by kernels_vec.hip and the block form of the
// four-launch smoother iteration (kernels_block_fused.hip).  Moved here verbatim from kernels_vec.hip.
#pragma once
#include "common.h"

// ---------------------------------------------------------------------------------------------------------------------
// reductions: two-stage (RED_BLOCKS partials, then one block sums them in a fixed order) -> deterministic
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

template <int NV>
__device__ __forceinline__ void block_store_partials(double (&acc)[NV], double* __restrict__ partial) {
  __shared__ double red[4][NV];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const double s = wave_sum(acc[v]);
    if (lane == 0) red[wave][v] = s;
  }
  __syncthreads();
  if (threadIdx.x < NV)
    partial[(int64_t)blockIdx.x * RED_MAXV + threadIdx.x] =
        red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

// every thread of the block gets out[v] = sum_{b < nblocks <= RED_BLOCKS} partial[b][v], summed in one fixed order: all
// blocks of a launch (and the kernels that follow) see the identical value, and no separate reduction launch is needed
template <int NV>
__device__ __forceinline__ void block_reduce_partials(const double* __restrict__ partial, int nblocks, double (&out)[NV]) {
  __shared__ double red2[4][NV];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    double s = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += 256) s += partial[(int64_t)b * RED_MAXV + v];
    s = wave_sum(s);
    if (lane == 0) red2[wave][v] = s;
  }
  __syncthreads();
#pragma unroll
  for (int v = 0; v < NV; ++v) out[v] = (red2[0][v] + red2[1][v]) + (red2[2][v] + red2[3][v]);
}

// a lane reads entry PAIRS of vectors that start on a 16-byte boundary: one 16-byte load per vector and iteration
typedef double vec_d2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ vec_d2 ld2(const double* p, int64_t i2) { return reinterpret_cast<const vec_d2*>(p)[i2]; }
__device__ __forceinline__ void st2(double* p, int64_t i2, vec_d2 v) { reinterpret_cast<vec_d2*>(p)[i2] = v; }
__host__ inline bool vec2_ok(const void* a, const void* b, int64_t stride) {
  return (stride & 1) == 0 && ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0;
}
