// The index planners behind alfi_patches_set, alfi_patches_set_groups and alfi_patches_set_multiplicative: host arrays in, a
// struct of tables out.  Plain host C++ (standard library only, no device): the device library uploads what they return, the
// host library exports them for the CPU tests (alfi_host_plan_*, tests/test_patch_plan.py).
//
// A planner returns 0, or PLAN_E_ARG (= ALFI_E_ARG of the C ABI) with the message in *err.
#pragma once
#include <algorithm>
#include <climits>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>
#include "cond_layout.h"

// (internal to whichever library includes this: nothing here is exported)
#pragma GCC visibility push(hidden)

constexpr int PLAN_E_ARG = -2;
constexpr int SMALL_PATCH_MAX = 160;   // register-resident inversion / one wave per patch up to here
constexpr int PATCH_MAX = 4096;        // blocked matrix-core inversion / one workgroup per patch beyond
constexpr int COND_LDS_MAX_BYTES = 150 * 1024;   // LDS a workgroup of the condensed apply may ask for
constexpr int COND_GROUP_MAX = 64;               // entries of a group, and skeleton entries coupled to one
constexpr int COND_CHUNK_PAIRS = 256;            // row pairs of X / W and of B per CondChunk: a lane per pair
constexpr int MULT_WAVE_NODES = 64;              // nodes of a patch that one wave sweeps (rows of a patch in SweepPlan::rowtab)

inline int plan_fail(std::string* err, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (err) *err = buf;
  return PLAN_E_ARG;
}

// the n entries at pd are whole nodes of bs components each: (node * bs, node * bs + 1, ...), node after node
inline bool patch_of_whole_nodes(int bs, const int32_t* pd, int64_t n) {
  if (bs <= 0 || n % bs != 0) return false;
  for (int64_t i = 0; i < n; i += bs)
    for (int c = 0; c < bs; ++c)
      if (pd[i + c] != (pd[i] / bs) * bs + c) return false;
  return true;
}

// ---- the patch layout (alfi_patches_set) -----------------------------------------------------------------------------------
struct PatchLayout {
  std::vector<int64_t> patch_ptr;    // (npatch+1) copies of the planner's input, made by who keeps the layout (the level:
  std::vector<int32_t> patch_dofs;   // (sum_n)    later calls read them on the host); the planner leaves them alone
  std::vector<int64_t> inv_ptr;      // (npatch+1) offsets of the dense inverses: n x ld, ld = n rounded up to even, padded to 16 doubles
  std::vector<int64_t> stage_ptr;    // (npatch+1) offsets into the staging buffer (ld slots per patch)
  std::vector<int32_t> dof_ptr;      // (n+1) CSR dof -> staged positions, in patch order (the fixed summation order)
  std::vector<int32_t> dof_pos;      // (sum_n)
  int64_t sum_n = 0, sum_n2 = 0, inv_doubles = 0, stage_len = 0;
  int max_np = 0;

  // what later calls read on the host stays (patch_ptr, patch_dofs, inv_ptr and the scalars); the tables that live on the
  // device go
  void release_tables() {
    std::vector<int64_t>().swap(stage_ptr);
    std::vector<int32_t>().swap(dof_ptr);
    std::vector<int32_t>().swap(dof_pos);
  }
};

inline int plan_patch_layout(int64_t n, int64_t npatch, const int64_t* pptr, const int32_t* pdofs, int patch_max,
                             PatchLayout* out, std::string* err) {
  const int64_t sum_n = npatch > 0 ? pptr[npatch] : 0;
  if (sum_n > INT32_MAX) return plan_fail(err, "too many patch dofs for int32 staging indices");
  std::vector<int64_t> inv_ptr(npatch + 1), stage_ptr(npatch + 1);
  int64_t ip = 0, sp = 0, sum_n2 = 0;
  int max_np = 0;
  for (int64_t p = 0; p < npatch; ++p) {
    const int64_t np = pptr[p + 1] - pptr[p];
    if (np <= 0 || np > patch_max)
      return plan_fail(err, "patch %lld has %lld dofs; supported range is 1..%d", (long long)p, (long long)np, patch_max);
    for (int64_t q = pptr[p]; q < pptr[p + 1]; ++q) {
      if (pdofs[q] < 0 || pdofs[q] >= n) return plan_fail(err, "patch %lld: dof %d out of range", (long long)p, pdofs[q]);
      if (q > pptr[p] && pdofs[q] <= pdofs[q - 1])
        return plan_fail(err, "patch %lld: dofs must be strictly ascending", (long long)p);
    }
    const int64_t ld = (np + 1) & ~(int64_t)1;
    inv_ptr[p] = ip;
    stage_ptr[p] = sp;
    ip += (np * ld + 15) & ~(int64_t)15;
    sp += ld;
    sum_n2 += np * np;
    max_np = std::max<int>(max_np, (int)np);
  }
  inv_ptr[npatch] = ip;
  stage_ptr[npatch] = sp;
  if (sp > INT32_MAX) return plan_fail(err, "staging buffer exceeds int32 indexing");
  // dof -> staged positions (counting sort; patch order = fixed summation order)
  std::vector<int32_t> dof_ptr(n + 1, 0), dof_pos(sum_n > 0 ? sum_n : 1);
  for (int64_t q = 0; q < sum_n; ++q) dof_ptr[pdofs[q] + 1]++;
  for (int64_t i = 0; i < n; ++i) dof_ptr[i + 1] += dof_ptr[i];
  {
    std::vector<int32_t> fill(dof_ptr.begin(), dof_ptr.end() - 1);
    for (int64_t p = 0; p < npatch; ++p)
      for (int64_t q = pptr[p]; q < pptr[p + 1]; ++q)
        dof_pos[fill[pdofs[q]]++] = (int32_t)(stage_ptr[p] + (q - pptr[p]));
  }
  out->inv_ptr = std::move(inv_ptr);
  out->stage_ptr = std::move(stage_ptr);
  out->dof_ptr = std::move(dof_ptr);
  out->dof_pos = std::move(dof_pos);
  out->sum_n = sum_n;
  out->sum_n2 = sum_n2;
  out->max_np = max_np;
  out->inv_doubles = ip;
  out->stage_len = sp;
  return 0;
}

// ---- storage of one dense inverse: row pieces (the kernels that stream it: row_piece.h) --------------------------------------
// An n x n inverse with its rows padded to ld (n rounded up to min_rows, pad rows stored as zeros) is cut into row pieces: as
// many 128-row pieces as fit, then the binary digits of the remainder (64, 32, ..., min_rows).  A piece of R rows is stored
// [column][R] contiguously and the pieces follow each other, so the inverse is ld * n contiguous values that the apply streams
// front to back exactly once, a lane reading min_rows rows of one column as one aligned 16-byte load and a wave instruction
// 1 KiB of consecutive bytes.  Offset of entry (r, c), r < ld, c < n:
ALFI_HD inline int64_t piece_index(int r, int c, int n, int ld, int min_rows) {
  int row0 = r & ~127, rows = 128;
  if (row0 + 128 > ld) {
    const int rem = ld - row0;
    int rr = r - row0;
    for (int bit = 64; bit >= min_rows; bit >>= 1) {
      if (rem & bit) {
        if (rr < bit) {
          rows = bit;
          break;
        }
        rr -= bit;
        row0 += bit;
      }
    }
  }
  return (int64_t)row0 * n + (int64_t)c * rows + (r - row0);
}
// FP64 storage: min_rows = 2, ld = n rounded up to even (the caller passes it), patch p at inv + inv_ptr[p] (a multiple of 16
// doubles = 128 B)
ALFI_HD inline int64_t patch_inv_index(int r, int c, int n, int ld) { return piece_index(r, c, n, ld, 2); }

// FP32 storage (alfi_patches_set_storage, alfi_patches_set_macro_storage): min_rows = F32_ROWS -- the same 16 bytes per lane --,
// patch p at inv32 + f32_ptr[p], every patch on a 128-byte line
constexpr int F32_ROWS = 4;               // rows of a column per lane: one 16-byte load
constexpr int F32_ALIGN = 32;             // floats: a patch's storage starts on a 128-byte line

ALFI_HD inline int f32_ld(int n) { return (n + F32_ROWS - 1) & ~(F32_ROWS - 1); }
// floats patch p occupies (its padded rows, rounded up to whole 128-byte lines)
ALFI_HD inline int64_t f32_patch_floats(int n) { return ((int64_t)n * f32_ld(n) + F32_ALIGN - 1) & ~(int64_t)(F32_ALIGN - 1); }
ALFI_HD inline int64_t f32_inv_index(int r, int c, int n) { return piece_index(r, c, n, f32_ld(n), F32_ROWS); }
// (npatch + 1) offsets in floats; returns the floats of the level
inline int64_t plan_f32_offsets(int64_t npatch, const int64_t* pptr, std::vector<int64_t>* f32_ptr) {
  f32_ptr->resize((size_t)npatch + 1);
  int64_t ip = 0;
  for (int64_t p = 0; p < npatch; ++p) {
    (*f32_ptr)[(size_t)p] = ip;
    ip += f32_patch_floats((int)(pptr[p + 1] - pptr[p]));
  }
  (*f32_ptr)[(size_t)npatch] = ip;
  return ip;
}
// The ranges of patches an FP32 level of big patches is factored in, through an FP64 work buffer of `cap` doubles
// (alfi_ctx_set_f32_work_bytes).  Greedy: the longest run of consecutive patches whose FP64 row pieces (inv_ptr: the npatch + 1
// offsets of PatchLayout) fit the cap; one patch above the cap is a range of its own.  ranges: the boundaries, 0 = r_0 < r_1 <
// ... = npatch (no patches: 0 alone); returns the doubles of the largest range -- what the buffer must hold.
inline int64_t plan_f32_ranges(int64_t npatch, const int64_t* inv_ptr, int64_t cap, std::vector<int64_t>* ranges) {
  ranges->assign(1, 0);
  int64_t work = 0;
  for (int64_t p0 = 0; p0 < npatch;) {
    int64_t p1 = p0 + 1;
    while (p1 < npatch && inv_ptr[p1 + 1] - inv_ptr[p0] <= cap) ++p1;
    work = std::max(work, inv_ptr[p1] - inv_ptr[p0]);
    ranges->push_back(p1);
    p0 = p1;
  }
  return work;
}

// ---- the macro stars' apply (big_apply_kernel, kernels_bigpatch.hip; its block form, kernels_block_big.hip) ------------------
// workgroups per patch: enough of them to fill 256 CUs several times over, but no more waves than 128-row pieces
inline int big_split(int64_t npatch, int max_np) {
  const int64_t want = (2048 + npatch - 1) / npatch;
  const int pieces = (max_np + 127) / 128;
  const int cap = (pieces + 3) / 4;
  return (int)(want < 1 ? 1 : (want > cap ? cap : want));
}

// ---- the condensed layout (alfi_patches_set_groups; the tables of CondDev, common.h) ---------------------------------------
struct CondPlan {
  // per patch entry, condensed order [groups | skeleton]
  std::vector<int32_t> dofs, slot;
  // per group (gptr: the groups of patch p)
  std::vector<int64_t> gptr, g_mat, g_sidx;
  std::vector<int32_t> g_off, g_m, g_sc, g_uoff, g_xp, g_bp;
  std::vector<int32_t> sidx;
  // per patch
  std::vector<int32_t> p_nI, order;
  std::vector<int64_t> sptr, sinv_ptr, uptr, xp_ptr, bp_ptr;
  std::vector<int32_t> s_uptr, s_uidx, u_dst;
  // sigma chunks (chptr: the chunks of patch p), row pairs, group chunks (gcptr: the chunks of patch p)
  std::vector<int64_t> chptr, gcptr;
  std::vector<int32_t> ch_patch, ch_row, xp_grp, bp_grp;
  std::vector<CondChunk> gc;
  int64_t ngroups = 0, mat_doubles = 0, sinv_doubles = 0;
  int lds_bytes = 0, lds_front = 0, lds_back = 0, lds_gfront = 0, lds_gback = 0;
  int max_s = 0;       // largest skeleton
  int max_m = 0;       // largest group: <= 16 -> four groups per wave in the factorisation (cond_group16_kernel)
  int max_pairs = 0;   // most row pairs of X / W or of B in one patch: waves per patch of cond_front / cond_back
  int front_waves = 1; // most waves the early-load front kernel needs for one patch (cond_ahead_front_waves, cond_layout.h)
  int max_xpairs = 0;  // most row pairs of X / W in one patch, and
  int max_sc = 0;      // most coupled skeleton entries of one group: the tail launch (cond_tail, cond_layout.h)
  int umax = 0;

  // what later calls read on the host stays (sptr, gptr, chptr, gcptr and the scalars); the tables that live on the device go
  void release_tables() {
    CondPlan keep;
    keep.sptr.swap(sptr); keep.gptr.swap(gptr); keep.chptr.swap(chptr); keep.gcptr.swap(gcptr);
    keep.ngroups = ngroups; keep.mat_doubles = mat_doubles; keep.sinv_doubles = sinv_doubles;
    keep.lds_bytes = lds_bytes; keep.lds_front = lds_front; keep.lds_back = lds_back;
    keep.lds_gfront = lds_gfront; keep.lds_gback = lds_gback;
    keep.max_s = max_s; keep.max_m = max_m; keep.max_pairs = max_pairs; keep.front_waves = front_waves; keep.umax = umax;
    keep.max_xpairs = max_xpairs; keep.max_sc = max_sc;
    *this = std::move(keep);
  }
};

// group: one label per entry of pd (< 0: skeleton).  rowptr / colidx: block sparsity (nb block rows; the sign bit of a column
// index may carry the row-start mark of the flat layout and is masked).  sigma_rows: rows of inv(Sigma) per sigma chunk.
inline int plan_condensed(int bs, int64_t nb, int64_t npatch, const int64_t* pp, const int32_t* pd, const int32_t* group,
                          const int32_t* rowptr, const int32_t* colidx, int sigma_rows, CondPlan* out, std::string* err) {
  const int64_t sum_n = pp[npatch];
  std::vector<int32_t> c_dofs(sum_n), c_slot(sum_n), g_off, g_m, g_sc, g_uoff, sidx, p_nI(npatch), s_uptr, s_uidx;
  std::vector<int64_t> gptr(npatch + 1, 0), g_mat, g_sidx, sptr(npatch + 1, 0), sinv_ptr(npatch + 1, 0);
  std::vector<int32_t> node_pos(nb, -1);               // node -> condensed NODE position inside the current patch
  int64_t mat_off = 0, sinv_off = 0;
  int lds_max = 0, umax = 0, smax = 0;
  s_uptr.push_back(0);
  for (int64_t p = 0; p < npatch; ++p) {
    const int64_t off = pp[p];
    const int n = (int)(pp[p + 1] - off);
    if (n % bs != 0) return plan_fail(err, "patch %lld: condensed factors need patches of whole nodes", (long long)p);
    const int nn = n / bs;
    // labels per node; groups = distinct non-negative labels in ascending order
    std::vector<int32_t> lab(nn);
    bool one_label = patch_of_whole_nodes(bs, pd + off, n);
    for (int i = 0; i < nn; ++i) {
      lab[i] = group[off + (int64_t)i * bs];
      for (int c = 0; c < bs; ++c)
        if (group[off + (int64_t)i * bs + c] != lab[i]) one_label = false;
    }
    if (!one_label)
      return plan_fail(err, "patch %lld: entries of a node must be adjacent and carry one group label", (long long)p);
    std::vector<int32_t> labels;
    for (int i = 0; i < nn; ++i) if (lab[i] >= 0) labels.push_back(lab[i]);
    std::sort(labels.begin(), labels.end());
    labels.erase(std::unique(labels.begin(), labels.end()), labels.end());
    const int ng = (int)labels.size();
    // condensed node order: groups (ascending label, ascending node), then the skeleton nodes
    std::vector<int32_t> order;                         // condensed node position -> sorted node position
    order.reserve(nn);
    std::vector<int32_t> gstart(ng + 1, 0);
    for (int g = 0; g < ng; ++g) {
      for (int i = 0; i < nn; ++i) if (lab[i] == labels[g]) order.push_back(i);
      gstart[g + 1] = (int32_t)order.size();
    }
    const int nIn = (int)order.size();                  // interior nodes
    for (int i = 0; i < nn; ++i) if (lab[i] < 0) order.push_back(i);
    for (int q = 0; q < nn; ++q) {
      node_pos[pd[off + (int64_t)order[q] * bs] / bs] = q;
      for (int c = 0; c < bs; ++c) {
        c_dofs[off + (int64_t)q * bs + c] = pd[off + (int64_t)order[q] * bs + c];
        c_slot[off + (int64_t)q * bs + c] = order[q] * bs + c;
      }
    }
    const int sn = nn - nIn, s = sn * bs;
    p_nI[p] = nIn * bs;
    sptr[p + 1] = sptr[p] + s;
    const int64_t ld_s = (s + 1) & ~1;
    sinv_ptr[p] = sinv_off;
    sinv_off += ((int64_t)s * ld_s + 15) & ~(int64_t)15;
    if (s > smax) smax = s;
    gptr[p + 1] = gptr[p] + ng;
    // per group: the skeleton nodes its rows couple to; a column inside another group is an error
    std::vector<std::vector<int32_t>> row_contrib(sn);  // skeleton node -> (u position of its first component) per group
    int uoff = 0;
    std::vector<char> mark(sn);
    for (int g = 0; g < ng; ++g) {
      std::fill(mark.begin(), mark.end(), 0);
      for (int q = gstart[g]; q < gstart[g + 1]; ++q) {
        const int node = pd[off + (int64_t)order[q] * bs] / bs;
        for (int32_t k = rowptr[node]; k < rowptr[node + 1]; ++k) {
          const int cq = node_pos[colidx[k] & 0x7fffffff];
          if (cq < 0) continue;
          if (cq >= nIn) mark[cq - nIn] = 1;
          else if (cq < gstart[g] || cq >= gstart[g + 1])
            return plan_fail(err, "patch %lld: groups %d and another one are coupled by an operator entry "
                             "(a group may touch the rest of the patch only through unlabelled dofs)", (long long)p, labels[g]);
        }
      }
      const int m = (gstart[g + 1] - gstart[g]) * bs;
      int scn = 0;
      g_sidx.push_back((int64_t)sidx.size());
      for (int j = 0; j < sn; ++j)
        if (mark[j]) {
          for (int c = 0; c < bs; ++c) sidx.push_back(j * bs + c);
          row_contrib[j].push_back(uoff + scn * bs);
          ++scn;
        }
      const int sc = scn * bs;
      if (m > COND_GROUP_MAX || sc > COND_GROUP_MAX)
        return plan_fail(err, "patch %lld: group %d holds %d entries coupled to %d skeleton entries; the "
                         "condensed factors handle at most 64 of each", (long long)p, labels[g], m, sc);
      g_off.push_back(gstart[g] * bs);
      g_m.push_back(m);
      g_sc.push_back(sc);
      g_uoff.push_back(uoff);
      g_mat.push_back(mat_off);
      mat_off += cond_group_doubles(m, sc);
      uoff += sc;
    }
    if (uoff > umax) umax = uoff;
    for (int j = 0; j < sn; ++j)
      for (int c = 0; c < bs; ++c) {
        for (int32_t u : row_contrib[j]) s_uidx.push_back(u + c);
        s_uptr.push_back((int32_t)s_uidx.size());
      }
    for (int i = 0; i < nn; ++i) node_pos[pd[off + (int64_t)i * bs] / bs] = -1;
    const int lds = (n + uoff + s + 2) * (int)sizeof(double);
    if (lds > lds_max) lds_max = lds;
  }
  sinv_ptr[npatch] = sinv_off;
  if (lds_max > COND_LDS_MAX_BYTES) return plan_fail(err, "condensed apply would need %d bytes of LDS per patch", lds_max);
  if (g_off.empty()) return plan_fail(err, "no group label >= 0: nothing to condense");
  if (sidx.empty()) sidx.push_back(0);
  if (s_uidx.empty()) s_uidx.push_back(0);
  // dispatch order of a full-range apply: descending factor bytes (group matrices + inv(Sigma)), ties by index
  std::vector<int32_t> order((size_t)npatch);
  {
    std::vector<int64_t> pbytes((size_t)npatch, 0);
    for (int64_t p = 0; p < npatch; ++p) {
      const int64_t s = sptr[p + 1] - sptr[p];
      pbytes[p] = s * s;
      for (int64_t g = gptr[p]; g < gptr[p + 1]; ++g) pbytes[p] += cond_group_doubles(g_m[g], g_sc[g]);
    }
    for (int64_t p = 0; p < npatch; ++p) order[p] = (int32_t)p;
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return pbytes[a] > pbytes[b]; });
  }
  // tables of the three-launch apply (the big-patch kernels): chunks of <= sigma_rows rows of inv(Sigma) for the sigma kernel,
  // row pairs of the group matrices, the row-sorted order of the u buffer
  std::vector<int32_t> ch_patch, ch_row, xp_grp, bp_grp, g_xp(g_m.size()), g_bp(g_m.size()), u_dst;
  std::vector<int64_t> chptr((size_t)npatch + 1, 0), uptr((size_t)npatch + 1, 0), xp_ptr((size_t)npatch + 1, 0),
      bp_ptr((size_t)npatch + 1, 0);
  int lds_front = 0, lds_back = 0, max_pairs = 0, max_xpairs = 0, front_waves = 1;
  for (int64_t p = 0; p < npatch; ++p) {
    const int s = (int)(sptr[p + 1] - sptr[p]), ld = (s + 1) & ~1;
    for (int r = 0; r < ld; r += sigma_rows) {
      ch_patch.push_back((int32_t)p);
      ch_row.push_back(r);
    }
    chptr[p + 1] = (int64_t)ch_patch.size();
    int uo = 0, xp = 0, bp = 0;
    for (int64_t g = gptr[p]; g < gptr[p + 1]; ++g) {
      g_xp[g] = xp;
      g_bp[g] = bp;
      for (int i = 0; i < cond_pairs(g_m[g]); ++i) xp_grp.push_back((int32_t)g);
      for (int j = 0; j < cond_pairs(g_sc[g]); ++j) bp_grp.push_back((int32_t)g);
      xp += cond_pairs(g_m[g]);
      bp += cond_pairs(g_sc[g]);
      uo += g_sc[g];
    }
    uptr[p + 1] = uptr[p] + uo;
    xp_ptr[p + 1] = xp_ptr[p] + xp;
    bp_ptr[p + 1] = bp_ptr[p] + bp;
    // every entry of the u buffer is one contribution to one skeleton row: s_uidx restricted to the patch is a permutation
    const int32_t qb = s_uptr[sptr[p]], qe = s_uptr[sptr[p + 1]];
    if (qe - qb != uo) return plan_fail(err, "patch %lld: inconsistent skeleton contributions", (long long)p);
    u_dst.resize((size_t)uptr[p + 1]);
    for (int32_t q = qb; q < qe; ++q) u_dst[uptr[p] + s_uidx[q]] = q - qb;
    max_pairs = std::max(max_pairs, std::max(xp, bp));
    max_xpairs = std::max(max_xpairs, xp);
    front_waves = std::max(front_waves, cond_ahead_front_waves(xp, bp));
    lds_front = std::max(lds_front, (int)((pp[p + 1] - pp[p] + p_nI[p] + uo + 2) * (int64_t)sizeof(double)));
    lds_back = std::max(lds_back, (int)((s + uo + 2) * (int64_t)sizeof(double)));
  }
  if (ch_patch.empty()) { ch_patch.push_back(0); ch_row.push_back(0); }
  if (xp_grp.empty()) xp_grp.push_back(0);
  if (bp_grp.empty()) bp_grp.push_back(0);
  if (u_dst.empty()) u_dst.push_back(0);
  if (lds_front > COND_LDS_MAX_BYTES) return plan_fail(err, "condensed apply would need %d bytes of LDS per patch", lds_front);
  // chunks of consecutive groups: at most COND_CHUNK_PAIRS row pairs of X / W and of B each (a lane per pair), one descriptor
  // per chunk (CondChunk, cond_layout.h)
  std::vector<CondChunk> gc;
  std::vector<int64_t> gcptr((size_t)npatch + 1, 0), stage_off((size_t)npatch + 1, 0);
  for (int64_t p = 0; p < npatch; ++p)          // the staging layout of plan_patch_layout: ld_p = n_p rounded up to even
    stage_off[p + 1] = stage_off[p] + ((pp[p + 1] - pp[p] + 1) & ~(int64_t)1);
  int lds_gf = 0, lds_gb = 0;
  for (int64_t p = 0; p < npatch; ++p) {
    int64_t g = gptr[p];
    while (g < gptr[p + 1]) {
      CondChunk c;
      const int64_t ga = g;
      int xp = 0, bp = 0, ne = 0, nu = 0;
      while (g < gptr[p + 1] && xp + cond_pairs(g_m[g]) <= COND_CHUNK_PAIRS && bp + cond_pairs(g_sc[g]) <= COND_CHUNK_PAIRS) {
        xp += cond_pairs(g_m[g]);
        bp += cond_pairs(g_sc[g]);
        ne += g_m[g];
        nu += g_sc[g];
        ++g;
      }
      c.off = pp[p]; c.ubase = uptr[p]; c.sidx0 = g_sidx[ga]; c.stage_off = stage_off[p];
      c.xq0 = (int32_t)(xp_ptr[p] + g_xp[ga]); c.xq1 = c.xq0 + xp;
      c.bq0 = (int32_t)(bp_ptr[p] + g_bp[ga]); c.bq1 = c.bq0 + bp;
      c.e0 = g_off[ga]; c.ne = ne; c.u0 = g_uoff[ga]; c.nu = nu; c.nI = p_nI[p]; c.pad = 0;
      c.xp0 = (int32_t)xp_ptr[p]; c.bp0 = (int32_t)bp_ptr[p];
      gc.push_back(c);
      lds_gf = std::max(lds_gf, (int)(2 * ne * sizeof(double)));
      lds_gb = std::max(lds_gb, (int)(nu * sizeof(double)));
    }
    gcptr[p + 1] = (int64_t)gc.size();
  }
  if (xp_ptr[npatch] > INT32_MAX || bp_ptr[npatch] > INT32_MAX)
    return plan_fail(err, "condensed factors: too many row pairs on one level");
  if (gc.empty()) gc.push_back(CondChunk());
  CondPlan& o = *out;
  o.ngroups = (int64_t)g_off.size();
  o.mat_doubles = mat_off;
  o.sinv_doubles = sinv_off;
  o.lds_bytes = lds_max;
  o.lds_front = lds_front;
  o.lds_back = lds_back;
  o.lds_gfront = lds_gf + 16;
  o.lds_gback = lds_gb + 16;
  o.max_s = smax;
  o.max_m = g_m.empty() ? 0 : *std::max_element(g_m.begin(), g_m.end());
  o.max_pairs = max_pairs;
  o.front_waves = front_waves;
  o.max_xpairs = max_xpairs;
  o.max_sc = g_sc.empty() ? 0 : *std::max_element(g_sc.begin(), g_sc.end());
  o.umax = umax;
  o.dofs = std::move(c_dofs); o.slot = std::move(c_slot);
  o.gptr = std::move(gptr); o.g_mat = std::move(g_mat); o.g_sidx = std::move(g_sidx);
  o.g_off = std::move(g_off); o.g_m = std::move(g_m); o.g_sc = std::move(g_sc); o.g_uoff = std::move(g_uoff);
  o.g_xp = std::move(g_xp); o.g_bp = std::move(g_bp);
  o.sidx = std::move(sidx);
  o.p_nI = std::move(p_nI); o.order = std::move(order);
  o.sptr = std::move(sptr); o.sinv_ptr = std::move(sinv_ptr); o.uptr = std::move(uptr);
  o.xp_ptr = std::move(xp_ptr); o.bp_ptr = std::move(bp_ptr);
  o.s_uptr = std::move(s_uptr); o.s_uidx = std::move(s_uidx); o.u_dst = std::move(u_dst);
  o.chptr = std::move(chptr); o.gcptr = std::move(gcptr);
  o.ch_patch = std::move(ch_patch); o.ch_row = std::move(ch_row); o.xp_grp = std::move(xp_grp); o.bp_grp = std::move(bp_grp);
  o.gc = std::move(gc);
  return 0;
}

// ---- the sweep schedule (alfi_patches_set_multiplicative) ------------------------------------------------------------------
struct SweepPlan {
  bool big = false;                // a patch holds more than MULT_WAVE_NODES nodes or small_max dofs: workgroup-per-patch sweep
  std::vector<int32_t> seq;        // (nit) patch ids, wavefront-major
  std::vector<int64_t> wave_ptr;   // (nwave+1) offsets into seq
  // persistent schedule of the whole apply (forward sweep, then -- symmetrised -- the wavefronts in reverse): item -> patch,
  // predecessor counts (the last writers of the nodes an item reads), successor lists
  std::vector<int32_t> items, pred0, succ_ptr, succ;
  int32_t nitems = 0;              // = items.size()
  std::vector<int32_t> rowtab;     // (npatch, MULT_WAVE_NODES, 3) first block, block count, node of every patch node (!big)
};

// the arguments of a sweep that need no sparsity: patches of whole nodes (the sweep works on block rows), the iteration set in
// range.  *big: up to MULT_WAVE_NODES nodes and small_max dofs a wave sweeps a patch, beyond (macro stars) a workgroup does.
inline int check_sweep(int bs, int64_t npatch, const int64_t* pp, const int32_t* pd, int small_max, int64_t nit,
                       const int64_t* iterset, bool* big, std::string* err) {
  *big = false;
  for (int64_t p = 0; p < npatch; ++p) {
    const int64_t a = pp[p], b = pp[p + 1];
    if (b - a > small_max || (b - a) / bs > MULT_WAVE_NODES) *big = true;
    if ((b - a) % bs != 0) return plan_fail(err, "patch %lld: multiplicative sweeps need patches of whole nodes", (long long)p);
    if (!patch_of_whole_nodes(bs, pd + a, b - a)) return plan_fail(err, "patch %lld does not consist of whole nodes", (long long)p);
  }
  for (int64_t t = 0; t < nit; ++t)
    if (iterset[t] < 0 || iterset[t] >= npatch) return plan_fail(err, "iteration set entry out of range");
  return 0;
}

// Arguments as check_sweep has passed them (big: its verdict).  Fails only at the int32 limits of the persistent schedule; seq,
// wave_ptr and rowtab are complete then.
inline int plan_sweep(int bs, int64_t nb, int64_t npatch, const int64_t* pp, const int32_t* pd, const int32_t* rowptr,
                      const int32_t* colidx, int64_t nit, const int64_t* iterset, bool symmetrise, bool big, SweepPlan* out,
                      std::string* err) {
  out->big = big;
  // wavefront of position t = 1 + max wavefront of earlier positions whose patch holds a node in the closure of patch t
  // (closure = columns of the patch's block rows).  node_wave[c] = last wavefront that wrote node c.
  std::vector<int32_t> node_wave(nb, -1), wave_of(nit);
  int32_t nwave = 0;
  for (int64_t t = 0; t < nit; ++t) {
    const int64_t p = iterset[t];
    const int64_t a = pp[p], b = pp[p + 1];
    int32_t w = -1;
    for (int64_t q = a; q < b; q += bs) {
      const int32_t node = pd[q] / bs;
      for (int32_t k = rowptr[node]; k < rowptr[node + 1]; ++k) {
        const int32_t c = colidx[k] & 0x7fffffff;
        if (node_wave[c] > w) w = node_wave[c];
      }
    }
    ++w;
    wave_of[t] = w;
    if (w + 1 > nwave) nwave = w + 1;
    for (int64_t q = a; q < b; q += bs) node_wave[pd[q] / bs] = w;
  }
  // counting sort of the positions by wavefront (stable)
  std::vector<int64_t>& wave_ptr = out->wave_ptr;
  wave_ptr.assign(nwave + 1, 0);
  for (int64_t t = 0; t < nit; ++t) wave_ptr[wave_of[t] + 1]++;
  for (int32_t w = 0; w < nwave; ++w) wave_ptr[w + 1] += wave_ptr[w];
  std::vector<int32_t>& seq = out->seq;
  seq.resize(nit);
  {
    std::vector<int64_t> fill(wave_ptr.begin(), wave_ptr.end() - 1);
    for (int64_t t = 0; t < nit; ++t) seq[fill[wave_of[t]]++] = (int32_t)iterset[t];
  }
  // ---- the persistent schedule: items = the forward sweep in wavefront-major order, then (symmetrised) the wavefronts in
  // reverse order, each in its listed order -- exactly the launch sequence of the per-wavefront schedule.
  // Predecessors of an item = the LAST WRITERS (earlier items) of the nodes it reads: patches writing the same node conflict
  // with each other, so earlier writers are ordered before the last one transitively; a patch that READS a node this item
  // writes has, by the symmetric sparsity, nodes in this item's closure, whose last writer is that patch or a later conflicting
  // one.  The list order is a topological order of these dependencies.
  if (!big) {
    // row table of the sweep kernels (mult_wg_rows): per patch node its first block, block count and node
    std::vector<int32_t>& rowtab = out->rowtab;
    rowtab.assign((size_t)npatch * MULT_WAVE_NODES * 3, 0);
    for (int64_t p = 0; p < npatch; ++p) {
      const int64_t a = pp[p], b = pp[p + 1];
      for (int64_t q = a, i = 0; q < b; q += bs, ++i) {
        const int32_t node = pd[q] / bs;
        int32_t* rt = &rowtab[((size_t)p * MULT_WAVE_NODES + (size_t)i) * 3];
        rt[0] = rowptr[node];
        rt[1] = rowptr[node + 1] - rowptr[node];
        rt[2] = node;
      }
    }
  }
  std::vector<int32_t> items(seq);
  if (symmetrise)
    for (int32_t w = nwave - 1; w >= 0; --w)
      for (int64_t q = wave_ptr[w]; q < wave_ptr[w + 1]; ++q) items.push_back(seq[q]);
  const int64_t N = (int64_t)items.size();
  if (N > INT32_MAX / 2) return plan_fail(err, "iteration set too long for the persistent schedule");
  std::vector<int32_t> last_writer(nb, -1), pred0(N, 0), tmp;
  std::vector<int32_t> e_from, e_to;               // the dependencies as (pred, item) pairs to keep memory flat
  e_from.reserve((size_t)N * 32);
  e_to.reserve((size_t)N * 32);
  for (int64_t t = 0; t < N; ++t) {
    const int64_t p = items[t];
    const int64_t a = pp[p], b = pp[p + 1];
    tmp.clear();
    for (int64_t q = a; q < b; q += bs) {
      const int32_t node = pd[q] / bs;
      for (int32_t k = rowptr[node]; k < rowptr[node + 1]; ++k) {
        const int32_t lw = last_writer[colidx[k] & 0x7fffffff];
        if (lw >= 0) tmp.push_back(lw);
      }
    }
    std::sort(tmp.begin(), tmp.end());
    tmp.erase(std::unique(tmp.begin(), tmp.end()), tmp.end());
    pred0[t] = (int32_t)tmp.size();
    for (int32_t f : tmp) {
      e_from.push_back(f);
      e_to.push_back((int32_t)t);
    }
    for (int64_t q = a; q < b; q += bs) last_writer[pd[q] / bs] = (int32_t)t;
  }
  if (e_from.size() > (size_t)INT32_MAX) return plan_fail(err, "too many dependencies for int32 offsets");
  std::vector<int32_t> succ_ptr(N + 1, 0), succ(e_from.size() > 0 ? e_from.size() : 1);
  for (int32_t f : e_from) succ_ptr[f + 1]++;
  for (int64_t t = 0; t < N; ++t) succ_ptr[t + 1] += succ_ptr[t];
  {
    std::vector<int32_t> fill(succ_ptr.begin(), succ_ptr.end() - 1);
    for (size_t e = 0; e < e_from.size(); ++e) succ[fill[e_from[e]]++] = e_to[e];
  }
  out->items = std::move(items);
  out->pred0 = std::move(pred0);
  out->succ_ptr = std::move(succ_ptr);
  out->succ = std::move(succ);
  out->nitems = (int32_t)N;
  return 0;
}

// ---- sweeps that read condensed factors (alfi_patches_set_multiplicative_condensed) -------------------------------------------
// The work lists of one dependency wavefront w of a sweep over condensed patches: what the chunked condensed launches
// (cond_gfront / cond_gsigma / cond_gback, kernels_bigpatch.hip) and the residual launch take in place of a patch range.
struct SweepCondPlan {
  std::vector<int64_t> wk_ptr, wc_ptr, wn_ptr;   // (nwave+1) offsets into gchunk, schunk, node
  std::vector<int32_t> gchunk;   // group chunks (indices into CondPlan::gc): [gcptr[p], gcptr[p+1]) of the wavefront's patches, seq order
  std::vector<int32_t> schunk;   // sigma chunks (indices into ch_patch / ch_row): the same over chptr
  std::vector<int32_t> node;     // the block rows of the wavefront's patches, patch after patch: the rows of the residual
};

// seq / wave_ptr: SweepPlan's; gcptr / chptr: CondPlan's; the patches as check_sweep has passed them (whole nodes).  The reverse
// pass of a symmetrised sweep walks the same wavefronts backwards: no second table.
inline int plan_sweep_condensed(int bs, int64_t npatch, const int64_t* pp, const int32_t* pd, int64_t nwave,
                                const int64_t* wave_ptr, const int32_t* seq, const int64_t* gcptr, const int64_t* chptr,
                                SweepCondPlan* out, std::string* err) {
  if (npatch > 0 && (gcptr[npatch] > INT32_MAX || chptr[npatch] > INT32_MAX))
    return plan_fail(err, "condensed sweeps: too many chunks for int32 lists");
  SweepCondPlan& o = *out;
  o.wk_ptr.assign((size_t)nwave + 1, 0);
  o.wc_ptr.assign((size_t)nwave + 1, 0);
  o.wn_ptr.assign((size_t)nwave + 1, 0);
  o.gchunk.clear();
  o.schunk.clear();
  o.node.clear();
  for (int64_t w = 0; w < nwave; ++w) {
    for (int64_t t = wave_ptr[w]; t < wave_ptr[w + 1]; ++t) {
      const int64_t p = seq[t];
      if (p < 0 || p >= npatch) return plan_fail(err, "condensed sweeps: sequence entry out of range");
      for (int64_t k = gcptr[p]; k < gcptr[p + 1]; ++k) o.gchunk.push_back((int32_t)k);   // (none: a patch without interior group)
      for (int64_t c = chptr[p]; c < chptr[p + 1]; ++c) o.schunk.push_back((int32_t)c);
      for (int64_t q = pp[p]; q < pp[p + 1]; q += bs) o.node.push_back(pd[q] / bs);
    }
    o.wk_ptr[(size_t)w + 1] = (int64_t)o.gchunk.size();
    o.wc_ptr[(size_t)w + 1] = (int64_t)o.schunk.size();
    o.wn_ptr[(size_t)w + 1] = (int64_t)o.node.size();
  }
  return 0;
}

#pragma GCC visibility pop
