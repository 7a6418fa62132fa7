// Group labels for condensed patch factors, found from the block sparsity of the level alone (alfi_patches_find_groups): the
// callers of the PCPATCH boundary hand over patches, never labels.  Plain host C++ (no HIP): libalfi_hip.so calls it on the
// level's own sparsity, libalfi_host.so exports it for the CPU tests (alfi_host_find_groups).
//
// Per patch, on the node graph restricted to the patch (an edge where either of the two block rows holds the other node):
//   * hubs = nodes coupled to EVERY node of the patch (the centre vertex of a star): skeleton; H = the graph without them;
//   * the other nodes are visited in ascending (degree in H, position in the patch); an unassigned seed s proposes
//       {s} + {u in N_H(s), unassigned, N_H[u] a subset of N_H[s]}          (closed neighbourhoods: the nodes s dominates),
//     accepted with >= 2 nodes, <= 64 dofs, <= 64 coupled skeleton dofs, and no member adjacent in H to an accepted group
//     (groups touch each other only through the skeleton: what alfi_patches_set_groups validates);
//   * everything else is skeleton (-1);
//   * the groups of a patch are kept only if  sum_g (m_g^2 + 2 m_g s_g) + s^2  <=  0.75 n^2  doubles, else the whole patch is -1.
// In a [P2+FB]^3 vertex star (51 nodes; the link of the centre is a cube with face centres) every face-centre edge node
// dominates the 4 face bubbles of its spokes: 6 mutually uncoupled groups of 15 dofs, each coupled to 27 of the 63 skeleton dofs
// -- 10 179 doubles against 23 409.  [P1+FB]^3 stars have no dominated nodes and stay dense.
// Deterministic: the order depends on degrees and positions only.  Patches that are not whole nodes get -1.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>
#include "patch_plan.h"   // patch_of_whole_nodes

// rowptr / colidx: block sparsity (nb block rows; the sign bit of a column index may carry the row-start mark of the flat
// layout and is masked).  out: one label per entry of pdofs.  Returns the number of patches that got groups.
inline int64_t alfi_find_groups_host(int bs, int64_t nb, int64_t npatch, const int64_t* pp, const int32_t* pd,
                                     const int32_t* rowptr, const int32_t* colidx, int32_t* out) {
  std::vector<int32_t> node_pos((size_t)(nb > 0 ? nb : 1), -1);
  std::vector<uint64_t> adj, nh;
  std::vector<int32_t> lab, order, cand;
  std::vector<int> hdeg;
  std::vector<char> hub, blocked;
  int64_t npatch_grouped = 0;
  auto popcount = [](uint64_t v) { return (int)__builtin_popcountll(v); };
  for (int64_t p = 0; p < npatch; ++p) {
    const int64_t off = pp[p];
    const int n = (int)(pp[p + 1] - off);
    for (int i = 0; i < n; ++i) out[off + i] = -1;
    if (!patch_of_whole_nodes(bs, pd + off, n)) continue;
    const int nn = n / bs;
    if (nn < 3) continue;
    const int W = (nn + 63) / 64;
    adj.assign((size_t)nn * W, 0);
    for (int i = 0; i < nn; ++i) node_pos[pd[off + (int64_t)i * bs] / bs] = i;
    for (int i = 0; i < nn; ++i) {
      const int32_t node = pd[off + (int64_t)i * bs] / bs;
      for (int32_t k = rowptr[node]; k < rowptr[node + 1]; ++k) {
        const int32_t c = colidx[k] & 0x7fffffff;
        if (c < 0 || c >= nb) continue;
        const int j = node_pos[c];
        if (j < 0 || j == i) continue;
        adj[(size_t)i * W + (j >> 6)] |= (uint64_t)1 << (j & 63);
        adj[(size_t)j * W + (i >> 6)] |= (uint64_t)1 << (i & 63);
      }
    }
    for (int i = 0; i < nn; ++i) node_pos[pd[off + (int64_t)i * bs] / bs] = -1;
    // hubs, and the neighbourhoods in H
    hub.assign(nn, 0);
    for (int i = 0; i < nn; ++i) {
      int d = 0;
      for (int w = 0; w < W; ++w) d += popcount(adj[(size_t)i * W + w]);
      hub[i] = d == nn - 1;
    }
    nh = adj;
    hdeg.assign(nn, 0);
    for (int i = 0; i < nn; ++i) {
      for (int j = 0; j < nn; ++j)
        if (hub[j] || hub[i]) nh[(size_t)i * W + (j >> 6)] &= ~((uint64_t)1 << (j & 63));
      for (int w = 0; w < W; ++w) hdeg[i] += popcount(nh[(size_t)i * W + w]);
    }
    order.clear();
    for (int i = 0; i < nn; ++i)
      if (!hub[i]) order.push_back(i);
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return hdeg[a] < hdeg[b]; });
    lab.assign(nn, -1);
    blocked.assign(nn, 0);                          // adjacent in H to a member of an accepted group
    int ng = 0;
    int64_t cond_doubles = 0;
    int nI = 0;
    for (int32_t s : order) {
      if (lab[s] >= 0) continue;
      const uint64_t* ns = &nh[(size_t)s * W];
      cand.clear();
      cand.push_back(s);
      for (int u = 0; u < nn; ++u) {
        if (u == s || !((ns[u >> 6] >> (u & 63)) & 1) || lab[u] >= 0) continue;
        // N_H[u] inside N_H[s]: u itself is a neighbour of s; its neighbours must be s or neighbours of s
        const uint64_t* nu = &nh[(size_t)u * W];
        bool inside = true;
        for (int w = 0; w < W && inside; ++w) {
          uint64_t closed_s = ns[w];
          if ((s >> 6) == w) closed_s |= (uint64_t)1 << (s & 63);
          if (nu[w] & ~closed_s) inside = false;
        }
        if (inside) cand.push_back(u);
      }
      if (cand.size() < 2 || (int)cand.size() * bs > 64) continue;
      std::sort(cand.begin(), cand.end());
      bool ok = true;
      for (int32_t u : cand)
        if (blocked[u]) ok = false;
      if (!ok) continue;
      // the skeleton nodes the candidate couples to: every neighbour (in the patch graph, hubs included) outside it
      int scn = 0;
      for (int j = 0; j < nn; ++j) {
        if (std::binary_search(cand.begin(), cand.end(), (int32_t)j)) continue;
        bool touch = false;
        for (int32_t u : cand)
          if ((adj[(size_t)u * W + (j >> 6)] >> (j & 63)) & 1) touch = true;
        if (touch) ++scn;
      }
      if (scn * bs > 64) continue;
      for (int32_t u : cand) lab[u] = ng;
      for (int32_t u : cand)
        for (int j = 0; j < nn; ++j)
          if ((nh[(size_t)u * W + (j >> 6)] >> (j & 63)) & 1) blocked[j] = 1;
      ++ng;
      const int64_t m = (int64_t)cand.size() * bs, sc = (int64_t)scn * bs;
      cond_doubles += m * m + 2 * m * sc;
      nI += (int)m;
    }
    if (ng == 0) continue;
    const int64_t s = n - nI;
    cond_doubles += s * s;
    if (4 * cond_doubles > 3 * (int64_t)n * n) continue;      // not worth it: the patch stays one dense Schur complement
    for (int i = 0; i < nn; ++i)
      for (int c = 0; c < bs; ++c) out[off + (int64_t)i * bs + c] = lab[i];
    ++npatch_grouped;
  }
  return npatch_grouped;
}
