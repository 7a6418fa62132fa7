// Block right-hand sides on levels of the four-launch smoother iteration (smooth_fgmres_fused, api_smoother.hip): the kernels of
// that iteration for 2 .. BLOCK_NV = 4 columns, with the launches per iteration of one column.
//
// The contract is that of kernels_block.hip: column c of a result is the single-vector kernel's result on column c BIT FOR BIT.
// Every kernel here is its single-vector original (kernels_patch.hip: patch_apply_il_kernel; kernels_vec.hip: the rest) with the
// per-column state held NV times or, on the BLAS-1 side, with the column slot on blockIdx.y and the original decomposition on
// blockIdx.x: per column the same products and the same sums in the same order, __builtin_fma where the original has one and
// plain + where it has that.  What is loaded once for the columns: the interleaved small-patch inverses, the operator values,
// colflag, rowptr, dof_ptr / dof_pos and the Dirichlet mask.
//
// Slot s of the level's block workspace (common.h: blk_ws, blk_part) belongs to column cols.c[s] of the
// caller's operands; only the first and the last kernel touch those.
#include "common.h"
#include "hs_layout.h"
#include "block_cols.h"
#include "reduce.h"
#include "load_pair.h"

// ---------------------------------------------------------------------------------------------------------------------
// stage 1 from the interleaved copy (patch_apply_il_kernel): G lanes per patch, 64 / G patches per wave.  The v[2G] pairs of
// the lane's row pair are loaded once; x_p is gathered, and the shuffle + fma chain runs, per column in the original order.
// stage[c * stage_len + stage_ptr[p] + r] = sum_j inv_p[r][j] * X[c * ldx + dofs_p[j]]
// ---------------------------------------------------------------------------------------------------------------------
template <int G, bool NT, int NV>
__global__ __launch_bounds__(256) void patch_apply_il_block_kernel(int64_t p0, int64_t p1, int nc,
                                                                    const int64_t* __restrict__ patch_ptr,
                                                                    const int32_t* __restrict__ patch_dofs,
                                                                    const int64_t* __restrict__ stage_ptr,
                                                                    const double* __restrict__ il,
                                                                    const double* __restrict__ X, int64_t ldx,
                                                                    double* __restrict__ stage, int64_t stage_len) {
  constexpr int PW = 64 / G, LW = PW * G;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t w = p0 / PW + (int64_t)blockIdx.x * 4 + wave;     // wave group; the grid covers [p0 / PW, (p1 - 1) / PW]
  const int q = lane / G, l = lane - q * G;
  const int64_t p = w * PW + q;
  const bool inwave = lane < LW && w * PW < p1;                    // the group exists (its storage is allocated whole)
  const bool live = inwave && p >= p0 && p < p1;
  int n = 0;
  int64_t off = 0;
  if (live) {
    off = patch_ptr[p];
    n = (int)(patch_ptr[p + 1] - off);
  }
  double xa[NV], xb[NV];   // x_p[l], x_p[l + G] of every column
#pragma unroll
  for (int s = 0; s < NV; ++s) xa[s] = xb[s] = 0.0;
  if (l < n) {
    const int64_t d = patch_dofs[off + l];
#pragma unroll
    for (int s = 0; s < NV; ++s) xa[s] = X[(int64_t)s * ldx + d];
  }
  if (l + G < n) {
    const int64_t d = patch_dofs[off + l + G];
#pragma unroll
    for (int s = 0; s < NV; ++s) xb[s] = X[(int64_t)s * ldx + d];
  }
  // all nc columns of the lane's row pair are requested before the first one is used
  const double* base = il + ((w * nc) * (int64_t)LW + lane) * 2;
  double2 v[2 * G];
#pragma unroll
  for (int c = 0; c < 2 * G; ++c)
    v[c] = (inwave && c < nc) ? load_pair<NT>(base + (int64_t)c * (2 * LW)) : make_double2(0.0, 0.0);
  double acc0[NV], acc1[NV];
#pragma unroll
  for (int s = 0; s < NV; ++s) acc0[s] = acc1[s] = 0.0;
  const int src0 = q * G;
#pragma unroll
  for (int c = 0; c < 2 * G; ++c) {
#pragma unroll
    for (int s = 0; s < NV; ++s) {
      const double xc = __shfl(c < G ? xa[s] : xb[s], src0 + (c < G ? c : c - G), 64);
      acc0[s] = __builtin_fma(v[c].x, xc, acc0[s]);
      acc1[s] = __builtin_fma(v[c].y, xc, acc1[s]);
    }
  }
  // rows >= n of the interleaved copy are zero, so storing the pair is valid whenever its first row exists (stage has ld slots)
  if (live && 2 * l < n) {
    double* dst = stage + stage_ptr[p] + 2 * l;
#pragma unroll
    for (int s = 0; s < NV; ++s) *reinterpret_cast<double2*>(dst + (int64_t)s * stage_len) = make_double2(acc0[s], acc1[s]);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// patch_sum_scale_kernel: per column c its own f = 1 / |w_c| from its own norm partials (a zero column: f = 0, z = v = 0
// exactly), z_c = f (sum of column c's staged patch results), v_c = f w_c; lane 0 of wave c of block 0 finishes column j - 1 of
// column c's Hessenberg (or starts its rotated rhs).  Column c's staged results are at stage.p[c]: slots of the level's block
// staging buffer, or the level's own staging buffer for a column that went through the single apply.
// ---------------------------------------------------------------------------------------------------------------------
struct BlockStage {
  const double* p[BLOCK_NV];
};

// block_reduce_partials<1> for column c of NV: out[c] = sum_b partial[c * pstride + b * RED_MAXV] in its order
template <int NV>
__device__ __forceinline__ void block_reduce_partials_cols(const double* __restrict__ partial, int64_t pstride, int nblocks,
                                                           double (&out)[NV]) {
  __shared__ double red2c[NV][4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int c = 0; c < NV; ++c) {
    double s = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += 256) s += partial[c * pstride + (int64_t)b * RED_MAXV];
    s = wave_sum(s);
    if (lane == 0) red2c[c][wave] = s;
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < NV; ++c) out[c] = (red2c[c][0] + red2c[c][1]) + (red2c[c][2] + red2c[c][3]);
}

template <int NV>
__global__ __launch_bounds__(256) void patch_sum_scale_block_kernel(int64_t n, const int32_t* __restrict__ dof_ptr,
                                                                     const int32_t* __restrict__ dof_pos, BlockStage stage,
                                                                     const uint8_t* __restrict__ bc_mask,
                                                                     const double* __restrict__ W, int64_t ldw,
                                                                     double* __restrict__ Z, int64_t zs, double* __restrict__ V,
                                                                     int64_t vs, const double* __restrict__ normpart,
                                                                     int64_t pstride, int nblocks, double* __restrict__ hs,
                                                                     int64_t hstride, int j, int K, int pou) {
  static_assert(NV <= 4, "one wave of the workgroup per column's Hessenberg");
  double s2[NV], f[NV];
  block_reduce_partials_cols<NV>(normpart, pstride, nblocks, s2);
  const HsLayout hl(K);
#pragma unroll
  for (int c = 0; c < NV; ++c) {
    const double tt = sqrt(s2[c]);
    f[c] = tt != 0.0 ? 1.0 / tt : 0.0;
    if (blockIdx.x == 0 && threadIdx.x == 64 * c) {
      double* hsc = hs + c * hstride;
      if (j == 0) {                       // beta = |r0|, rotated rhs = beta e_1
        hsc[hl.beta] = tt;
        hsc[hl.grs] = tt;
        for (int i = 1; i <= K; ++i) hsc[hl.grs + i] = 0.0;
      } else {
        hessenberg_column(hsc, K, j - 1, hsc + hl.hd, tt);
      }
    }
  }
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    double s[NV];
#pragma unroll
    for (int c = 0; c < NV; ++c) s[c] = 0.0;
    const int32_t q0 = dof_ptr[i], q1 = dof_ptr[i + 1];
    for (int32_t q = q0; q < q1; ++q) {
      const int32_t pos = dof_pos[q];
#pragma unroll
      for (int c = 0; c < NV; ++c) s[c] += stage.p[c][pos];
    }
    const bool bc = bc_mask[i] != 0;
#pragma unroll
    for (int c = 0; c < NV; ++c) {
      if (pou && q1 - q0 > 1) s[c] /= (double)(q1 - q0);
      const double wi = W[c * ldw + i];
      Z[c * zs + i] = f[c] * (bc ? wi : s[c]);   // Dirichlet dofs: the smoother copies its argument there
      V[c * vs + i] = f[c] * wi;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// bsr_spmv_dot_kernel for NC columns: W_c = A Z_c on the block rows of a flat-layout matrix, LPR lanes per block row, and in the
// same pass the partials of V_{c,v} . W_c, v < nvec <= NVEC, against column c's own Krylov basis.  One colflag load and one set
// of value loads per block serve the NC gathers; the NC row sums go through the same __shfl_xor tree.  NVEC is nvec rounded
// up (block_dot_vectors): an accumulator's arithmetic does not depend on how many others the instantiation holds, the guard
// keeps the loads inside the basis.  The dots stay in this launch: 4 columns x 16 vectors are 64 FP64 accumulators per lane,
// which the 512 registers of a lane at one workgroup of 256 threads per CU hold without scratch (the table in CHANGELOG); these
// levels are bound by dependent launches, not by occupancy, and a launch of their own for the dots would be a fifth one.
// ---------------------------------------------------------------------------------------------------------------------
typedef double fused_d2 __attribute__((ext_vector_type(2)));

template <int BS, int LPR, int NVEC, int NC>
__global__ __launch_bounds__(256) void bsr_spmv_dot_block_kernel(int64_t nbrows, const int32_t* __restrict__ rowptr,
                                                                  const int32_t* __restrict__ colflag,
                                                                  const double* __restrict__ vals, const double* __restrict__ Z,
                                                                  int64_t zs, double* __restrict__ W, int64_t ldw,
                                                                  const double* __restrict__ V, int64_t vs, int64_t stride,
                                                                  int nvec, double* __restrict__ partial, int64_t pstride) {
  constexpr int BB = BS * BS;
  const int l = threadIdx.x % LPR;
  double acc[NC][NVEC];
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int v = 0; v < NVEC; ++v) acc[c][v] = 0.0;
  for (int64_t row = ((int64_t)blockIdx.x * 256 + threadIdx.x) / LPR; row < nbrows;
       row += (int64_t)gridDim.x * (256 / LPR)) {
    double s[NC][BS];
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int r = 0; r < BS; ++r) s[c][r] = 0.0;
    const int32_t lo = rowptr[row], hi = rowptr[row + 1];
    for (int32_t k = lo + l; k < hi; k += LPR) {
      const int64_t col = colflag[k] & 0x7fffffff;
      const double* vb = vals + ((int64_t)k >> 6) * (64 * BB);
      const int kl = k & 63;
      double a[BB];
#pragma unroll
      for (int q = 0; q < BB / 2; ++q) {
        const fused_d2 t = *(reinterpret_cast<const fused_d2*>(vb + q * 128) + kl);
        a[2 * q] = t.x;
        a[2 * q + 1] = t.y;
      }
      if (BB & 1) a[BB - 1] = vb[(BB / 2) * 128 + kl];
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        double xv[BS];
#pragma unroll
        for (int cc = 0; cc < BS; ++cc) xv[cc] = Z[c * zs + col * BS + cc];
#pragma unroll
        for (int r = 0; r < BS; ++r)
#pragma unroll
          for (int cc = 0; cc < BS; ++cc) s[c][r] = __builtin_fma(a[r * BS + cc], xv[cc], s[c][r]);
      }
    }
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1)
#pragma unroll
      for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int r = 0; r < BS; ++r) s[c][r] += __shfl_xor(s[c][r], o);
    if (l == 0) {
#pragma unroll
      for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int r = 0; r < BS; ++r) {
          const int64_t i = row * BS + r;
          W[c * ldw + i] = s[c][r];
#pragma unroll
          for (int v = 0; v < NVEC; ++v)
            if (v < nvec) acc[c][v] = __builtin_fma(V[c * vs + v * stride + i], s[c][r], acc[c][v]);
        }
    }
  }
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    if (c > 0) __syncthreads();     // block_store_partials' LDS is read by wave 0 until here
    block_store_partials<NVEC>(acc[c], partial + c * pstride);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// the BLAS-1 side: the column slot on blockIdx.y, the original decomposition on blockIdx.x
// ---------------------------------------------------------------------------------------------------------------------
// the ternary chain keeps the column list in registers (a runtime index into a by-value array would go through memory)
__device__ __forceinline__ int block_col(const BlockCols& cols, int s) {
  return s == 0 ? cols.c[0] : s == 1 ? cols.c[1] : s == 2 ? cols.c[2] : cols.c[3];
}

// B != nullptr: x_c = 0 and w_s = b_c (the memset and copy_kernel of a zero guess), then -- either way -- the |w_s|^2 partials of
// multi_dot_kernel<1, true> with V = w
__global__ __launch_bounds__(256) void first_norm_block_kernel(const double* __restrict__ B, int64_t ldb, double* __restrict__ X,
                                                                int64_t ldx, BlockCols cols, double* __restrict__ W, int64_t ldw,
                                                                double* __restrict__ partial, int64_t pstride, int64_t n) {
  const int s = blockIdx.y;
  double* w = W + s * ldw;
  const int64_t n2 = n >> 1;
  const bool last = (n & 1) && blockIdx.x == gridDim.x - 1 && threadIdx.x == 255;     // the odd last entry
  if (B) {
    const int64_t c = block_col(cols, s);
    const double* b = B + c * ldb;
    double* x = X + c * ldx;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n2; i += (int64_t)gridDim.x * 256) {
      vec_d2 t;
      t.x = b[2 * i];
      t.y = b[2 * i + 1];
      st2(w, i, t);
      x[2 * i] = 0.0;
      x[2 * i + 1] = 0.0;
    }
    if (last) {
      w[n - 1] = b[n - 1];
      x[n - 1] = 0.0;
    }
  }
  // (each thread reads back exactly the entries it wrote)
  double acc[1] = {0.0};
#pragma unroll 2
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n2; i += (int64_t)gridDim.x * 256) {
    const vec_d2 wi = ld2(w, i);
    const vec_d2 a = ld2(w, i);
    acc[0] = __builtin_fma(a.y, wi.y, __builtin_fma(a.x, wi.x, acc[0]));
  }
  if (last) {
    const double wi = w[n - 1];
    acc[0] = __builtin_fma(w[n - 1], wi, acc[0]);
  }
  block_store_partials<1>(acc, partial + s * pstride);
}

// multi_axpy_norm_kernel<NV, true> with hblocks > 0 on slot blockIdx.y: h from the hblocks dot partials, w -= V h, |w|^2 partials
template <int NV>
__global__ __launch_bounds__(256) void multi_axpy_norm_block_kernel(const double* __restrict__ Vb, int64_t vs, int64_t stride,
                                                                     double* __restrict__ hb, int64_t hstride,
                                                                     double* __restrict__ Wb, int64_t ldw,
                                                                     double* __restrict__ partial, int64_t n,
                                                                     const double* __restrict__ hpart, int64_t pstride,
                                                                     int hblocks) {
  const int s = blockIdx.y;
  const double* V = Vb + s * vs;
  double* h = hb + s * hstride;
  double* w = Wb + s * ldw;
  double hv[NV];
  block_reduce_partials<NV>(hpart + s * pstride, hblocks, hv);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
#pragma unroll
    for (int v = 0; v < NV; ++v) h[v] = hv[v];
  }
  double acc[1] = {0.0};
  const int64_t n2 = n >> 1;
#pragma unroll 2
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n2; i += (int64_t)gridDim.x * 256) {
    vec_d2 wi = ld2(w, i);
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const vec_d2 a = ld2(V + v * stride, i);
      wi.x = __builtin_fma(-hv[v], a.x, wi.x);
      wi.y = __builtin_fma(-hv[v], a.y, wi.y);
    }
    st2(w, i, wi);
    acc[0] = __builtin_fma(wi.y, wi.y, __builtin_fma(wi.x, wi.x, acc[0]));
  }
  if ((n & 1) && blockIdx.x == gridDim.x - 1 && threadIdx.x == 255) {
    double wi = w[n - 1];
#pragma unroll
    for (int v = 0; v < NV; ++v) wi = __builtin_fma(-hv[v], V[v * stride + n - 1], wi);
    w[n - 1] = wi;
    acc[0] = __builtin_fma(wi, wi, acc[0]);
  }
  block_store_partials<1>(acc, partial + s * pstride);
}

// fgmres_finish_fused_kernel on slot blockIdx.y: column k - 1 of the Hessenberg from (h, partials of |w|^2), back substitution
__global__ __launch_bounds__(256) void fgmres_finish_fused_block_kernel(const double* __restrict__ normpart, int64_t pstride,
                                                                        int nblocks, double* __restrict__ hsb, int64_t hstride,
                                                                        int k, int K) {
  double s2[1];
  block_reduce_partials<1>(normpart + blockIdx.y * pstride, nblocks, s2);
  if (threadIdx.x != 0) return;
  HsLayout L(K);
  double* hs = hsb + blockIdx.y * hstride;
  hessenberg_column(hs, K, k - 1, hs + L.hd, sqrt(s2[0]));
  double* y = hs + L.y;
  const double* grs = hs + L.grs;
  for (int i = k - 1; i >= 0; --i) {
    double s = grs[i];
    for (int q = i + 1; q < k; ++q) s -= hs[L.H(q) + i] * y[q];
    const double d = hs[L.H(i) + i];
    y[i] = d != 0.0 ? s / d : 0.0;
  }
}

// multi_axpy_add_kernel<NV, VEC> on slot blockIdx.y: x_c += sum_v y_s[v] Z_{s,v}
template <int NV, bool VEC>
__global__ __launch_bounds__(256) void multi_axpy_add_block_kernel(const double* __restrict__ Zb, int64_t zs, int64_t stride,
                                                                    const double* __restrict__ yb, int64_t hstride,
                                                                    double* __restrict__ X, int64_t ldx, BlockCols cols,
                                                                    int64_t n) {
  const int s = blockIdx.y;
  const double* Z = Zb + s * zs;
  const double* y = yb + s * hstride;
  double* x = X + (int64_t)block_col(cols, s) * ldx;
  double yv[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) yv[v] = y[v];
  if (VEC) {
    const int64_t n2 = n >> 1;
#pragma unroll 2
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n2; i += (int64_t)gridDim.x * 256) {
      vec_d2 xi = ld2(x, i);
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        const vec_d2 a = ld2(Z + v * stride, i);
        xi.x = __builtin_fma(yv[v], a.x, xi.x);
        xi.y = __builtin_fma(yv[v], a.y, xi.y);
      }
      st2(x, i, xi);
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
      double xi = x[n - 1];
#pragma unroll
      for (int v = 0; v < NV; ++v) xi = __builtin_fma(yv[v], Z[v * stride + n - 1], xi);
      x[n - 1] = xi;
    }
  } else {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
      double xi = x[i];
#pragma unroll
      for (int v = 0; v < NV; ++v) xi = __builtin_fma(yv[v], Z[v * stride + i], xi);
      x[i] = xi;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// launch wrappers.  ws: the level's block workspace of nc slots (the caller has grown it); slot strides: KrylovWs, krylov_ws.h
// ---------------------------------------------------------------------------------------------------------------------
namespace {
struct Slots {
  int nc, K;
  int64_t n, ldv, vs, zs, hstride, pstride;
  double *V, *Z, *w, *hs, *part1, *part2;
};
Slots slots_of(const alfi_level* L, int nc) {
  Slots S;
  const KrylovWs& ws = L->blk_ws;
  S.nc = nc;
  S.K = ws.K;
  S.n = L->n;
  S.ldv = ws.ldv;
  S.vs = ws.vs();
  S.zs = ws.zs();
  S.hstride = ws.hstride();
  S.pstride = L->blk_part.per;
  S.V = ws.V;
  S.Z = ws.Z;
  S.w = ws.w;
  S.hs = ws.hs;
  S.part1 = L->blk_part.p;
  S.part2 = L->blk_part.p + block_partial_set(RED_BLOCKS, RED_MAXV);
  return S;
}
int check_slots(alfi_level* L, int nc) {
  if (nc < 2 || nc > BLOCK_NV || nc > L->blk_ws.slots || nc > L->blk_part.slots || L->blk_ws.K != L->ws.K)
    return alfi_set_error(L->ctx, ALFI_E_STATE, "block fused iteration on %d columns without its workspace", nc);
  return 0;
}
// the same grid as ew_grid (kernels_vec.hip)
dim3 fused_ew_grid(int64_t n, int nc) {
  int64_t b = (n + 255) / 256;
  if (b > 8192) b = 8192;
  if (b < 1) b = 1;
  return dim3((unsigned)b, (unsigned)nc);
}
}   // namespace

// stage 1 of a level that applies the interleaved copy, for the nc columns X + s * ldx: stage + s * lay.stage_len
int launch_patch_apply_il_block(alfi_level* L, int nc, const double* X, int64_t ldx, double* stage) {
  alfi_ctx* ctx = L->ctx;
  if (nc < 2 || nc > BLOCK_NV) return alfi_set_error(ctx, ALFI_E_ARG, "an interleaved block launch takes 2 .. %d columns", BLOCK_NV);
  if (!L->il_valid || L->held != HELD_F64) return alfi_set_error(ctx, ALFI_E_STATE, "interleaved block apply on a level without the copy");
  if (L->npatch <= 0) return 0;
  ProfScope prof(ctx, ALFI_EV_PATCH_APPLY);     // to the end of the function
  const int PW = 64 / L->il_G;
  const int64_t p0 = 0, p1 = L->npatch;
  const int64_t nwave = (p1 - 1) / PW - p0 / PW + 1;
  const dim3 igrid((unsigned)((nwave + 3) / 4)), block(256);
#define ALFI_ILB(GV, NVV)                                                                                                    \
  hipLaunchKernelGGL((patch_apply_il_block_kernel<GV, true, NVV>), igrid, block, 0, ctx->stream, p0, p1, L->il_nc,            \
                     L->patch_ptr, L->patch_dofs, L->stage_ptr, L->inv_il, X, ldx, stage, L->lay.stage_len)
#define ALFI_IL(GV)                       \
  case GV:                                \
    switch (nc) {                         \
      case 2: ALFI_ILB(GV, 2); break;     \
      case 3: ALFI_ILB(GV, 3); break;     \
      default: ALFI_ILB(GV, 4); break;    \
    }                                     \
    break;
  switch (L->il_G) {
    ALFI_IL(4) ALFI_IL(7) ALFI_IL(8) ALFI_IL(12) ALFI_IL(16)
    default: return alfi_set_error(ctx, ALFI_E_STATE, "interleaved patch storage with %d lanes per patch", L->il_G);
  }
#undef ALFI_IL
#undef ALFI_ILB
  ALFI_HIP_CHECK(ctx, hipGetLastError());
  return 0;
}

// w_s = b_c, x_c = 0 (B != nullptr) and the norm partials of every slot's w: red_blocks_for(n) of them in the first set
int launch_first_norm_block(alfi_level* L, const BlockCols& cols, const double* B, int64_t ldb, double* X, int64_t ldx) {
  alfi_ctx* ctx = L->ctx;
  ALFI_CHECK(check_slots(L, cols.n));
  const Slots S = slots_of(L, cols.n);
  if (S.n <= 0) return 0;
  hipLaunchKernelGGL(first_norm_block_kernel, dim3((unsigned)red_blocks_for(S.n), (unsigned)S.nc), dim3(256), 0, ctx->stream, B, ldb,
                     X, ldx, cols, S.w, S.ldv, S.part1, S.pstride, S.n);
  ALFI_HIP_CHECK(ctx, hipGetLastError());
  return 0;
}

// z_j, v_j and column j - 1 of the Hessenberg of every slot from the staged results at stage[s]; normpart: the set (0: the
// first, 1: the second) that holds the nblocks norm partials
int launch_patch_sum_scale_block(alfi_level* L, int nc, const double* const* stage, int normset, int nblocks, int j) {
  alfi_ctx* ctx = L->ctx;
  ALFI_CHECK(check_slots(L, nc));
  const Slots S = slots_of(L, nc);
  if (S.n <= 0) return 0;
  BlockStage st;
  for (int s = 0; s < BLOCK_NV; ++s) st.p[s] = stage[s < nc ? s : 0];
  const dim3 grid = fused_ew_grid(S.n, 1), block(256);
#define ALFI_PSS(NVV)                                                                                                          \
  hipLaunchKernelGGL((patch_sum_scale_block_kernel<NVV>), grid, block, 0, ctx->stream, S.n, L->dof_ptr, L->dof_pos, st,         \
                     L->bc_mask, S.w, S.ldv, S.Z + (int64_t)j * S.ldv, S.zs, S.V + (int64_t)j * S.ldv, S.vs,                     \
                     normset ? S.part2 : S.part1, S.pstride, nblocks, S.hs, S.hstride, j, S.K, L->pou ? 1 : 0)
  switch (nc) {
    case 2: ALFI_PSS(2); break;
    case 3: ALFI_PSS(3); break;
    default: ALFI_PSS(4); break;
  }
#undef ALFI_PSS
  ALFI_HIP_CHECK(ctx, hipGetLastError());
  return 0;
}

namespace {
template <int BS, int LPR, int NVEC>
int launch_spmv_dot_block_nc(alfi_ctx* ctx, const DevBSR& A, const Slots& S, int j, int nvec, int* nblocks) {
  const int64_t rows_per_block = 256 / LPR;
  int64_t g = (A.nbrows + rows_per_block - 1) / rows_per_block;
  if (g > RED_BLOCKS) g = RED_BLOCKS;      // one partial per block: at most RED_BLOCKS of them
  if (g < 1) g = 1;
  *nblocks = (int)g;
#define ALFI_SDB(NCC)                                                                                                          \
  hipLaunchKernelGGL((bsr_spmv_dot_block_kernel<BS, LPR, NVEC, NCC>), dim3((unsigned)g), dim3(256), 0, ctx->stream, A.nbrows,   \
                     A.rowptr, A.colidx, A.vals, S.Z + (int64_t)j * S.ldv, S.zs, S.w, S.ldv, S.V, S.vs, S.ldv, nvec, S.part1,    \
                     S.pstride)
  switch (S.nc) {
    case 2: ALFI_SDB(2); break;
    case 3: ALFI_SDB(3); break;
    default: ALFI_SDB(4); break;
  }
#undef ALFI_SDB
  ALFI_HIP_CHECK(ctx, hipGetLastError());
  return 0;
}
template <int BS, int LPR>
int launch_spmv_dot_block_lpr(alfi_ctx* ctx, const DevBSR& A, const Slots& S, int j, int nvec, int* nblocks) {
  switch (block_dot_vectors(nvec)) {
    case 4: return launch_spmv_dot_block_nc<BS, LPR, 4>(ctx, A, S, j, nvec, nblocks);
    case 8: return launch_spmv_dot_block_nc<BS, LPR, 8>(ctx, A, S, j, nvec, nblocks);
    case 16: return launch_spmv_dot_block_nc<BS, LPR, 16>(ctx, A, S, j, nvec, nblocks);
  }
  return alfi_set_error(ctx, ALFI_E_STATE, "block fused SpMV with %d dot vectors", nvec);
}
}   // namespace

// w_s = A z_{s,j} and the partials of V_s^T w_s (j + 1 vectors) into the first set; *nblocks = partials written per vector.
// The lanes per row are launch_bsr_spmv_dot's.
int launch_bsr_spmv_dot_block(alfi_level* L, int nc, int j, int* nblocks) {
  alfi_ctx* ctx = L->ctx;
  ALFI_CHECK(check_slots(L, nc));
  const Slots S = slots_of(L, nc);
  const DevBSR& A = L->A_own;
  const int nvec = j + 1;
  if (!A.flat || nvec < 1 || nvec > 16) return alfi_set_error(ctx, ALFI_E_STATE, "fused SpMV needs the flat layout and <= 16 vectors");
  const double avg = A.nbrows > 0 ? (double)A.nnzb / (double)A.nbrows : 0.0;
  if (A.bs == 2) {
    if (avg <= 12) return launch_spmv_dot_block_lpr<2, 4>(ctx, A, S, j, nvec, nblocks);
    if (avg <= 40) return launch_spmv_dot_block_lpr<2, 8>(ctx, A, S, j, nvec, nblocks);
    return launch_spmv_dot_block_lpr<2, 32>(ctx, A, S, j, nvec, nblocks);
  }
  if (A.bs == 3) {
    if (avg <= 24) return launch_spmv_dot_block_lpr<3, 8>(ctx, A, S, j, nvec, nblocks);
    if (avg <= 48) return launch_spmv_dot_block_lpr<3, 16>(ctx, A, S, j, nvec, nblocks);
    return launch_spmv_dot_block_lpr<3, 32>(ctx, A, S, j, nvec, nblocks);
  }
  return alfi_set_error(ctx, ALFI_E_ARG, "unsupported block size %d", A.bs);
}

// h_s from the hblocks dot partials of the first set, w_s -= V_s h_s, |w_s|^2 partials (red_blocks_for(n)) into the second set
int launch_multi_axpy_norm_block(alfi_level* L, int nc, int j, int hblocks) {
  alfi_ctx* ctx = L->ctx;
  ALFI_CHECK(check_slots(L, nc));
  const Slots S = slots_of(L, nc);
  const int nvec = j + 1;
  if (nvec < 1 || nvec > 16 || hblocks < 1) return alfi_set_error(ctx, ALFI_E_STATE, "block fused projection with %d vectors", nvec);
  if (!vec2_ok(S.V, S.w, S.ldv)) return alfi_set_error(ctx, ALFI_E_STATE, "block workspace off a 16-byte boundary");
  const dim3 grid((unsigned)red_blocks_for(S.n), (unsigned)nc), block(256);
  const int64_t hd = HsLayout(S.K).hd;
#define ALFI_CASE(N)                                                                                                           \
  case N:                                                                                                                      \
    hipLaunchKernelGGL((multi_axpy_norm_block_kernel<N>), grid, block, 0, ctx->stream, S.V, S.vs, S.ldv, S.hs + hd, S.hstride,  \
                       S.w, S.ldv, S.part2, S.n, S.part1, S.pstride, hblocks);                                                  \
    break;
  switch (nvec) {
    ALFI_CASE(1) ALFI_CASE(2) ALFI_CASE(3) ALFI_CASE(4) ALFI_CASE(5) ALFI_CASE(6) ALFI_CASE(7) ALFI_CASE(8) ALFI_CASE(9)
    ALFI_CASE(10) ALFI_CASE(11) ALFI_CASE(12) ALFI_CASE(13) ALFI_CASE(14) ALFI_CASE(15) ALFI_CASE(16)
  }
#undef ALFI_CASE
  ALFI_HIP_CHECK(ctx, hipGetLastError());
  return 0;
}

// column k - 1 of every slot's Hessenberg from the nblocks norm partials of the second set, its y; x_c += Z_s y_s
int launch_fgmres_finish_update_block(alfi_level* L, const BlockCols& cols, int k, int nblocks, double* X, int64_t ldx) {
  alfi_ctx* ctx = L->ctx;
  ALFI_CHECK(check_slots(L, cols.n));
  const Slots S = slots_of(L, cols.n);
  if (k < 1 || k > 16) return alfi_set_error(ctx, ALFI_E_STATE, "block fused update with %d vectors", k);
  hipLaunchKernelGGL(fgmres_finish_fused_block_kernel, dim3(1, (unsigned)S.nc), dim3(256), 0, ctx->stream, S.part2, S.pstride,
                     nblocks, S.hs, S.hstride, k, S.K);
  ALFI_HIP_CHECK(ctx, hipGetLastError());
  if (S.n <= 0) return 0;
  // (ldx is even, so every column of X is aligned as the first one is: one decision for the chunk, the single call's per column)
  const bool vec = vec2_ok(S.Z, X + (int64_t)cols.c[0] * ldx, S.ldv) && (ldx & 1) == 0;
  const dim3 grid = fused_ew_grid(vec ? (S.n + 1) / 2 : S.n, S.nc), block(256);
  const int64_t yo = HsLayout(S.K).y;
#define ALFI_CASE(N)                                                                                                           \
  case N:                                                                                                                      \
    if (vec)                                                                                                                   \
      hipLaunchKernelGGL((multi_axpy_add_block_kernel<N, true>), grid, block, 0, ctx->stream, S.Z, S.zs, S.ldv, S.hs + yo,      \
                         S.hstride, X, ldx, cols, S.n);                                                                        \
    else                                                                                                                       \
      hipLaunchKernelGGL((multi_axpy_add_block_kernel<N, false>), grid, block, 0, ctx->stream, S.Z, S.zs, S.ldv, S.hs + yo,     \
                         S.hstride, X, ldx, cols, S.n);                                                                        \
    break;
  switch (k) {
    ALFI_CASE(1) ALFI_CASE(2) ALFI_CASE(3) ALFI_CASE(4) ALFI_CASE(5) ALFI_CASE(6) ALFI_CASE(7) ALFI_CASE(8) ALFI_CASE(9)
    ALFI_CASE(10) ALFI_CASE(11) ALFI_CASE(12) ALFI_CASE(13) ALFI_CASE(14) ALFI_CASE(15) ALFI_CASE(16)
  }
#undef ALFI_CASE
  ALFI_HIP_CHECK(ctx, hipGetLastError());
  return 0;
}
