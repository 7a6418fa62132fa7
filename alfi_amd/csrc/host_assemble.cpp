// Host-side (CPU, OpenMP) operator generator for the synthetic ldc2d / ldc3d workloads.
//
// The reference obtains its level operators from Firedrake/TSFC/PyOP2 assembly of the UFL forms in
// alfi/solver.py:565-568 (velocity block of the Newton linearisation) and alfi/transfer.py:319-332 (the symmetric
// form used by the Schoeberl transfer).  Neither is available here, so this file assembles the same bilinear form
//
//     a(u, v) = nu (2 sym grad u, grad v) + gamma (cell_avg(div u), div v) + adv ((w . grad) u + (u . grad) w, v)
//
// for nodal vector elements on affine simplices directly into a block-CSR (block size d) matrix, from reference-cell
// tensors computed in alfi_amd/elements.py.  This is input generation (setup time), not part of the measured hot path.
//
// C ABI, plain pointers; called through ctypes from alfi_amd/_hostlib.py.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>
#include <omp.h>

#include "find_groups.h"
#include "patch_plan.h"

extern "C" {

// Node-to-node adjacency (two nodes are coupled iff they share a cell), sorted columns.
// Pass colidx == nullptr to only fill rowptr (counting pass).
int alfi_host_node_graph(int64_t ncell, int nloc, const int32_t* cell_nodes, int64_t nnode, int32_t* rowptr,
                         int32_t* colidx) {
  // node -> cells
  std::vector<int64_t> nptr(nnode + 1, 0);
  for (int64_t c = 0; c < ncell; ++c)
    for (int a = 0; a < nloc; ++a) nptr[cell_nodes[c * nloc + a] + 1]++;
  for (int64_t i = 0; i < nnode; ++i) nptr[i + 1] += nptr[i];
  std::vector<int32_t> ncells(nptr[nnode]);
  {
    std::vector<int64_t> fill(nptr.begin(), nptr.end() - 1);
    for (int64_t c = 0; c < ncell; ++c)
      for (int a = 0; a < nloc; ++a) ncells[fill[cell_nodes[c * nloc + a]]++] = (int32_t)c;
  }
  const bool counting = (colidx == nullptr);
  if (counting) rowptr[0] = 0;
#pragma omp parallel
  {
    std::vector<int32_t> buf;
#pragma omp for schedule(dynamic, 1024)
    for (int64_t i = 0; i < nnode; ++i) {
      buf.clear();
      for (int64_t p = nptr[i]; p < nptr[i + 1]; ++p) {
        const int32_t* cn = cell_nodes + (int64_t)ncells[p] * nloc;
        buf.insert(buf.end(), cn, cn + nloc);
      }
      std::sort(buf.begin(), buf.end());
      auto last = std::unique(buf.begin(), buf.end());
      int64_t cnt = last - buf.begin();
      if (counting)
        rowptr[i + 1] = (int32_t)cnt;
      else
        std::copy(buf.begin(), last, colidx + rowptr[i]);
    }
  }
  if (counting) {
    int64_t acc = 0;
    for (int64_t i = 0; i < nnode; ++i) {
      acc += rowptr[i + 1];
      if (acc > INT32_MAX) return -1;
      rowptr[i + 1] = (int32_t)acc;
    }
  }
  return 0;
}

static inline int64_t find_col(const int32_t* colidx, int64_t lo, int64_t hi, int32_t col) {
  const int32_t* p = std::lower_bound(colidx + lo, colidx + hi, col);
  return p - colidx;
}

// Element matrix Ae (ndof x ndof, dof = a*d + c) = nu*K + gamma*D + adv*N(w) of one affine simplex.
// gc: (d+1, d) gradients of the barycentric coordinates, vc: volume.  S: (nloc,nloc,d+1,d+1) avg d_i phi_a d_j phi_b;
// bI: (nloc,d+1) avg d_i phi_a; T1: (nloc,d+1,nloc,nloc) avg phi_k d_i phi_b phi_a (index order k,i,b,a);
// wk: (nloc, d) wind at the cell's nodes (only read when adv != 0).
struct ElemWork {
  std::vector<double> bvec, cki, t1, r, out, St;
  // S: (nloc, nloc, d+1, d+1), kept here transposed to (d+1, d+1, nloc, nloc)
  ElemWork(int nloc, int d, const double* S = nullptr)
      : bvec(nloc * d), cki((size_t)nloc * (d + 1)), t1((size_t)nloc * nloc), r((size_t)nloc * nloc * (d + 1) * d),
        out((size_t)(1 + d * d) * nloc * nloc), St((size_t)(d + 1) * (d + 1) * nloc * nloc) {
    const int nv = d + 1, nn = nloc * nloc;
    if (S)
      for (int ab = 0; ab < nn; ++ab)
        for (int ij = 0; ij < nv * nv; ++ij) St[(size_t)ij * nn + ab] = S[(size_t)ab * nv * nv + ij];
  }
};

// gfull: coefficient of the FULL grad-div term (div u, div v) of the Scott-Vogelius forms (alfi/solver.py:609-619,
// alfi/transfer.py:295-309), as opposed to gamma, the coefficient of the cell-averaged one of the PkP0 forms.
static void element_matrix(int nloc, int d, const double* gc, double vc, const double* S, const double* bI,
                           const double* T1, const double* wk, double nu, double gamma, double adv, ElemWork& W,
                           double* Ae, double gfull = 0.0) {
  const int nv = d + 1;
  const int ndof = nloc * d;
  double* bvec = W.bvec.data();
  double* cki = W.cki.data();
  if (nu != 0.0 || gfull != 0.0) {
    // out[q][ab] = sum_ij M[ij][q] St[ij][ab]: q = 0 the Gram entry g_i . g_j (-> G_ab), q = 1 + dd d + cc the product
    // g_i^dd g_j^cc (-> h[dd][cc] = int d_dd phi_a d_cc phi_b); the (a, b) index is innermost and contiguous in St
    const int nn = nloc * nloc, nq = 1 + d * d;
    double* out = W.out.data();
    std::fill(out, out + (size_t)nq * nn, 0.0);
    for (int i = 0; i < nv; ++i)
      for (int j = 0; j < nv; ++j) {
        const double* St = W.St.data() + (size_t)(i * nv + j) * nn;
        double m[10];
        double s = 0;
        for (int x = 0; x < d; ++x) s += gc[i * d + x] * gc[j * d + x];
        m[0] = s;
        for (int dd = 0; dd < d; ++dd)
          for (int cc = 0; cc < d; ++cc) m[1 + dd * d + cc] = gc[i * d + dd] * gc[j * d + cc];
        for (int q = 0; q < nq; ++q) {
          const double mq = m[q];
          double* oq = out + (size_t)q * nn;
#pragma omp simd
          for (int ab = 0; ab < nn; ++ab) oq[ab] += mq * St[ab];
        }
      }
    // K_(a,c),(b,dd) = delta_{c,dd} G_ab + int d_dd phi_a d_c phi_b ;  (div, div)_(a,c),(b,dd) = int d_c phi_a d_dd phi_b
    const double fn = nu * vc, fg = gfull * vc;
    for (int a = 0; a < nloc; ++a)
      for (int cc = 0; cc < d; ++cc) {
        double* row = Ae + (size_t)(a * d + cc) * ndof;
        for (int b = 0; b < nloc; ++b) {
          const int ab = a * nloc + b;
          for (int dd = 0; dd < d; ++dd) {
            double v = out[(size_t)(1 + dd * d + cc) * nn + ab];
            if (cc == dd) v += out[ab];
            row[b * d + dd] = fn * v + fg * out[(size_t)(1 + cc * d + dd) * nn + ab];
          }
        }
      }
  } else {
    std::fill(Ae, Ae + (size_t)ndof * ndof, 0.0);
  }
  if (gamma != 0.0) {
    for (int a = 0; a < nloc; ++a)
      for (int cc = 0; cc < d; ++cc) {
        double s = 0;
        for (int i = 0; i < nv; ++i) s += gc[i * d + cc] * bI[a * nv + i];
        bvec[a * d + cc] = s;  // (1/vol) int d_cc phi_a
      }
    const double f = gamma * vc;
    for (int p = 0; p < ndof; ++p) {
      const double bp = f * bvec[p];
      if (bp == 0.0) continue;
      for (int q = 0; q < ndof; ++q) Ae[(size_t)p * ndof + q] += bp * bvec[q];
    }
  }
  if (adv != 0.0) {
    // Both terms as small dense products with the (b, a) / a index innermost (contiguous in T1: the loops vectorise), then one
    // pass over Ae.  (Until round 5 the second term updated d x d entries of Ae per (b, i, k, a): 100 k dependent
    // read-modify-writes per cell, 4/5 of the time of the advective assembly.)
    //   t1[b][a]       = sum_{k,i} (w_k . g_i) T1[k,i,b,a]
    //   r[b][i][c][a]  = sum_k w_k^c T1[b,i,k,a]
    //   Ae[(a,c),(b,dd)] += adv vol (delta_{c,dd} t1[b][a] + sum_i r[b][i][c][a] g_i^dd)
    const int nn = nloc * nloc;
    double* t1 = W.t1.data();
    double* r = W.r.data();
    for (int k = 0; k < nloc; ++k)
      for (int i = 0; i < nv; ++i) {
        double s = 0;
        for (int x = 0; x < d; ++x) s += wk[k * d + x] * gc[i * d + x];
        cki[k * nv + i] = s;
      }
    std::fill(t1, t1 + nn, 0.0);
    for (int ki = 0; ki < nloc * nv; ++ki) {
      const double cc1 = cki[ki];
      const double* T = T1 + (size_t)ki * nn;  // T[b][a]
#pragma omp simd
      for (int q = 0; q < nn; ++q) t1[q] += cc1 * T[q];
    }
    std::fill(r, r + (size_t)nn * nv * d, 0.0);
    for (int bi = 0; bi < nloc * nv; ++bi) {
      const double* T = T1 + (size_t)bi * nn;  // T[k][a]
      double* rb = r + (size_t)bi * d * nloc;   // rb[c][a]
      for (int k = 0; k < nloc; ++k) {
        const double* Tk = T + k * nloc;
        for (int cc = 0; cc < d; ++cc) {
          const double wc = wk[k * d + cc];
          double* rc = rb + cc * nloc;
#pragma omp simd
          for (int a = 0; a < nloc; ++a) rc[a] += wc * Tk[a];
        }
      }
    }
    const double f = adv * vc;
    for (int a = 0; a < nloc; ++a)
      for (int cc = 0; cc < d; ++cc) {
        double* row = Ae + (size_t)(a * d + cc) * ndof;
        for (int b = 0; b < nloc; ++b) {
          double acc[3] = {0.0, 0.0, 0.0};
          for (int i = 0; i < nv; ++i) {
            const double rv = r[((size_t)(b * nv + i) * d + cc) * nloc + a];
            for (int dd = 0; dd < d; ++dd) acc[dd] += rv * gc[i * d + dd];
          }
          acc[cc] += t1[b * nloc + a];
          for (int dd = 0; dd < d; ++dd) row[b * d + dd] += f * acc[dd];
        }
      }
  }
}

// Cells in colour classes, no two cells of a class sharing a node (greedy, cells ascending): class k is
// cells[cptr[k] .. cptr[k + 1]), ascending.  Assembling one class at a time, its cells in parallel, no two threads add into
// the same block row and every operator entry is summed in the same order on every run, whatever the number of threads.
static void colour_cells(int64_t ncell, int nloc, const int32_t* cell_nodes, std::vector<int64_t>& cptr,
                         std::vector<int64_t>& cells) {
  int64_t nnode = 0;
  for (int64_t i = 0; i < ncell * nloc; ++i) nnode = std::max<int64_t>(nnode, (int64_t)cell_nodes[i] + 1);
  std::vector<int64_t> nptr(nnode + 1, 0);                 // node -> cells (ascending)
  for (int64_t i = 0; i < ncell * nloc; ++i) nptr[cell_nodes[i] + 1]++;
  for (int64_t i = 0; i < nnode; ++i) nptr[i + 1] += nptr[i];
  std::vector<int64_t> ncells(nptr[nnode]);
  {
    std::vector<int64_t> fill(nptr.begin(), nptr.end() - 1);
    for (int64_t c = 0; c < ncell; ++c)
      for (int a = 0; a < nloc; ++a) ncells[fill[cell_nodes[c * nloc + a]]++] = c;
  }
  std::vector<int32_t> colour(ncell);
  std::vector<int64_t> taken;                              // taken[k] == c: a neighbour of cell c has colour k
  for (int64_t c = 0; c < ncell; ++c) {
    for (int a = 0; a < nloc; ++a) {
      const int64_t n = cell_nodes[c * nloc + a];
      for (int64_t p = nptr[n]; p < nptr[n + 1] && ncells[p] < c; ++p) taken[colour[ncells[p]]] = c;
    }
    size_t k = 0;
    while (k < taken.size() && taken[k] == c) ++k;
    if (k == taken.size()) taken.push_back(-1);
    colour[c] = (int32_t)k;
  }
  cptr.assign(taken.size() + 1, 0);
  for (int64_t c = 0; c < ncell; ++c) cptr[colour[c] + 1]++;
  for (size_t k = 0; k < taken.size(); ++k) cptr[k + 1] += cptr[k];
  cells.resize(ncell);
  std::vector<int64_t> fill(cptr.begin(), cptr.end() - 1);
  for (int64_t c = 0; c < ncell; ++c) cells[fill[colour[c]]++] = c;
}

// vals (nnzb, d, d) += nu*K + gamma*D + adv*N(w), scattered into a BSR matrix whose block rows are the nodes mapped
// through row_map (nullptr: identity; row_map[node] < 0: row skipped) and whose block columns are all nodes.
// Deterministic: the cells are assembled colour class by colour class (colour_cells), without atomics.
int alfi_host_assemble_bsr(int64_t ncell, int nloc, int d, const int32_t* cell_nodes, const double* g,
                           const double* vol, const double* S, const double* bI, const double* T1, const double* w,
                           double nu, double gamma, double adv, const int32_t* row_map, const int32_t* rowptr,
                           const int32_t* colidx, double* vals, double gamma_full) {
  const int nv = d + 1;
  const int ndof = nloc * d;
  const bool do_adv = (adv != 0.0) && (w != nullptr);
  int err = 0;
  std::vector<int64_t> cptr, cells;
  colour_cells(ncell, nloc, cell_nodes, cptr, cells);
  const int64_t ncolour = (int64_t)cptr.size() - 1;
#pragma omp parallel
  {
    ElemWork W(nloc, d, S);
    std::vector<double> Ae((size_t)ndof * ndof), wk((size_t)nloc * d);
    for (int64_t k = 0; k < ncolour; ++k)
#pragma omp for schedule(dynamic, 256)
    for (int64_t i = cptr[k]; i < cptr[k + 1]; ++i) {
      const int64_t c = cells[i];
      const int32_t* cn = cell_nodes + c * nloc;
      if (row_map) {
        bool any = false;
        for (int a = 0; a < nloc; ++a) any |= row_map[cn[a]] >= 0;
        if (!any) continue;
      }
      if (do_adv)
        for (int k = 0; k < nloc; ++k)
          for (int x = 0; x < d; ++x) wk[k * d + x] = w[(int64_t)cn[k] * d + x];
      element_matrix(nloc, d, g + c * nv * d, vol[c], S, bI, T1, wk.data(), nu, gamma, do_adv ? adv : 0.0, W,
                     Ae.data(), gamma_full);
      for (int a = 0; a < nloc; ++a) {
        const int32_t ra = row_map ? row_map[cn[a]] : cn[a];
        if (ra < 0) continue;
        const int64_t lo = rowptr[ra], hi = rowptr[ra + 1];
        for (int b = 0; b < nloc; ++b) {
          const int64_t pos = find_col(colidx, lo, hi, cn[b]);
          if (pos >= hi || colidx[pos] != cn[b]) {
            err = 1;
            continue;
          }
          double* dst = vals + pos * d * d;
          for (int cc = 0; cc < d; ++cc)
            for (int dd = 0; dd < d; ++dd) dst[cc * d + dd] += Ae[(size_t)(a * d + cc) * ndof + b * d + dd];
        }
      }
    }
  }
  return err ? -2 : 0;
}

// Contributor lists for the DEVICE assembly of the level operators (csrc/kernels_assemble.hip): for every block (r, c) of the
// BSR sparsity the (cell, b * nloc + a) pairs with r = node a and c = node b of the cell, cells ascending and, inside a cell, b
// ascending -- a fixed order, so that the device sums every operator entry in the same order on every run (no atomics).
// cptr: (nnzb + 1) int64.  Call with ccell == nullptr to fill cptr only (counting pass).
// nindex >= nnode: cell_nodes may name nodes beyond the nnode rows of the sparsity (a rank's cells reach nodes it holds no
// operator row for); partial != 0: pairs whose block is not in the sparsity are skipped instead of being an error (ghost rows
// restricted to local columns).
int alfi_host_contributors(int64_t ncell, int nloc, const int32_t* cell_nodes, int64_t nnode, const int32_t* rowptr,
                           const int32_t* colidx, int64_t* cptr, int32_t* ccell, uint16_t* cba, int64_t nindex, int partial) {
  if (nindex < nnode) nindex = nnode;
  std::vector<int64_t> nptr(nindex + 1, 0);                 // node -> cells (ascending)
  for (int64_t c = 0; c < ncell; ++c)
    for (int a = 0; a < nloc; ++a) nptr[cell_nodes[c * nloc + a] + 1]++;
  for (int64_t i = 0; i < nindex; ++i) nptr[i + 1] += nptr[i];
  std::vector<int32_t> ncells(nptr[nindex]);
  {
    std::vector<int64_t> fill(nptr.begin(), nptr.end() - 1);
    for (int64_t c = 0; c < ncell; ++c)
      for (int a = 0; a < nloc; ++a) ncells[fill[cell_nodes[c * nloc + a]]++] = (int32_t)c;
  }
  const int64_t nnzb = rowptr[nnode];
  const bool counting = (ccell == nullptr);
  int err = 0;
  if (counting) std::fill(cptr, cptr + nnzb + 1, (int64_t)0);
  // the blocks of block row r are touched by the thread that owns r only: no atomics, a fixed order
#pragma omp parallel
  {
    std::vector<int64_t> cursor;
    std::vector<std::pair<int32_t, int64_t>> byc;        // the row's (column, block) pairs ascending: a rank's local operator
                                                         // numbers its columns owned-first, so its rows are not sorted
#pragma omp for schedule(dynamic, 512)
    for (int64_t r = 0; r < nnode; ++r) {
      const int64_t lo = rowptr[r], hi = rowptr[r + 1];
      if (!counting) cursor.assign(cptr + lo, cptr + hi);
      byc.resize((size_t)(hi - lo));
      for (int64_t k = lo; k < hi; ++k) byc[(size_t)(k - lo)] = std::make_pair(colidx[k], k);
      if (!std::is_sorted(byc.begin(), byc.end())) std::sort(byc.begin(), byc.end());
      for (int64_t q = nptr[r]; q < nptr[r + 1]; ++q) {
        const int32_t cell = ncells[q];
        const int32_t* cn = cell_nodes + (int64_t)cell * nloc;
        int a = 0;
        while (a < nloc && cn[a] != r) ++a;
        for (int b = 0; b < nloc; ++b) {
          const auto it = std::lower_bound(byc.begin(), byc.end(), std::make_pair(cn[b], (int64_t)-1));
          const int64_t pos = (it != byc.end() && it->first == cn[b]) ? it->second : hi;
          if (pos >= hi) {
            if (!partial) err = 1;
            continue;
          }
          if (counting) {
            cptr[pos + 1]++;
          } else {
            const int64_t at = cursor[pos - lo]++;
            ccell[at] = cell;
            cba[at] = (uint16_t)(b * nloc + a);
          }
        }
      }
    }
  }
  if (counting)
    for (int64_t k = 0; k < nnzb; ++k) cptr[k + 1] += cptr[k];
  return err ? -2 : 0;
}

// Dense interior blocks of the Schoeberl transfer, assembled directly: block `blk` (= coarse cell) receives the
// contributions of its nch children (fine cells blk*nch .. blk*nch+nch-1) restricted to the block's interior dofs.
// blk_local[node] = position of the node inside its block (0..m/d-1) or -1.  KII, DII: (nblk, m, m) row-major.
int alfi_host_interior_blocks(int64_t nblk, int nch, int nloc, int d, const int32_t* cell_nodes, const double* g,
                              const double* vol, const double* S, const double* bI, const int32_t* blk_local, int m,
                              double* KII, double* DII, int full_div) {
  const int nv = d + 1;
  const int ndof = nloc * d;
#pragma omp parallel
  {
    ElemWork W(nloc, d, S);
    std::vector<double> Ke((size_t)ndof * ndof), De((size_t)ndof * ndof);
#pragma omp for schedule(static)
    for (int64_t blk = 0; blk < nblk; ++blk) {
      double* Kb = KII + blk * m * m;
      double* Db = DII + blk * m * m;
      std::fill(Kb, Kb + (size_t)m * m, 0.0);
      std::fill(Db, Db + (size_t)m * m, 0.0);
      for (int ch = 0; ch < nch; ++ch) {
        const int64_t c = blk * nch + ch;
        const int32_t* cn = cell_nodes + c * nloc;
        element_matrix(nloc, d, g + c * nv * d, vol[c], S, bI, nullptr, nullptr, 1.0, 0.0, 0.0, W, Ke.data());
        element_matrix(nloc, d, g + c * nv * d, vol[c], S, bI, nullptr, nullptr, 0.0, full_div ? 0.0 : 1.0, 0.0, W,
                       De.data(), full_div ? 1.0 : 0.0);
        for (int a = 0; a < nloc; ++a) {
          const int la = blk_local[cn[a]];
          if (la < 0) continue;
          for (int b = 0; b < nloc; ++b) {
            const int lb = blk_local[cn[b]];
            if (lb < 0) continue;
            for (int cc = 0; cc < d; ++cc)
              for (int dd = 0; dd < d; ++dd) {
                const size_t src = (size_t)(a * d + cc) * ndof + b * d + dd;
                const size_t dst = (size_t)(la * d + cc) * m + lb * d + dd;
                Kb[dst] += Ke[src];
                Db[dst] += De[src];
              }
          }
        }
      }
    }
  }
  return 0;
}

// Transpose of a BSR matrix (counting sort; output columns ascending because rows are visited in order).
int alfi_host_bsr_transpose(int64_t nbrows, int64_t nbcols, int bs, const int32_t* rowptr, const int32_t* colidx,
                            const double* vals, int32_t* rowptr_t, int32_t* colidx_t, double* vals_t) {
  const int64_t nnzb = rowptr[nbrows];
  std::fill(rowptr_t, rowptr_t + nbcols + 1, 0);
  for (int64_t k = 0; k < nnzb; ++k) rowptr_t[colidx[k] + 1]++;
  for (int64_t j = 0; j < nbcols; ++j) rowptr_t[j + 1] += rowptr_t[j];
  std::vector<int32_t> fill(rowptr_t, rowptr_t + nbcols);
  std::vector<int32_t> src(nnzb);
  for (int64_t r = 0; r < nbrows; ++r)
    for (int64_t k = rowptr[r]; k < rowptr[r + 1]; ++k) {
      const int32_t q = fill[colidx[k]]++;
      colidx_t[q] = (int32_t)r;
      src[q] = (int32_t)k;
    }
  const int bb = bs * bs;
#pragma omp parallel for schedule(static)
  for (int64_t q = 0; q < nnzb; ++q) {
    const double* s = vals + (int64_t)src[q] * bb;
    double* t = vals_t + q * bb;
    for (int i = 0; i < bs; ++i)
      for (int j = 0; j < bs; ++j) t[j * bs + i] = s[i * bs + j];
  }
  return 0;
}

// Dirichlet rows and columns -> identity (what firedrake.assemble(a, bcs=...) produces).  bcmask: (all nodes * d) bytes.
// row_ids: node of each of the nrow block rows (a row subset, rank-local generation), or nullptr: row r is node r.
int alfi_host_apply_bc_bsr(int64_t nrow, int d, const int32_t* rowptr, const int32_t* colidx, double* vals,
                           const uint8_t* bcmask, const int32_t* row_ids) {
#pragma omp parallel for schedule(static)
  for (int64_t r = 0; r < nrow; ++r) {
    const int64_t rnode = row_ids ? row_ids[r] : r;
    for (int64_t p = rowptr[r]; p < rowptr[r + 1]; ++p) {
      const int64_t cnode = colidx[p];
      double* blk = vals + p * d * d;
      for (int cc = 0; cc < d; ++cc)
        for (int dd = 0; dd < d; ++dd) {
          const bool rb = bcmask[rnode * d + cc], cb = bcmask[cnode * d + dd];
          if (rb || cb) blk[cc * d + dd] = (rb && cb && rnode == cnode && cc == dd) ? 1.0 : 0.0;
        }
    }
  }
  return 0;
}

// Dense principal sub-blocks A[dofs_b, dofs_b] of a BSR matrix.  blk_ptr: (nblk+1) offsets into blk_dofs;
// out_ptr: (nblk+1) offsets into out (out_ptr[b+1]-out_ptr[b] == n_b^2), row-major blocks.
int alfi_host_extract_blocks(int d, const int32_t* rowptr, const int32_t* colidx, const double* vals, int64_t nblk,
                             const int64_t* blk_ptr, const int32_t* blk_dofs, const int64_t* out_ptr, double* out) {
#pragma omp parallel for schedule(dynamic, 64)
  for (int64_t b = 0; b < nblk; ++b) {
    const int32_t* dofs = blk_dofs + blk_ptr[b];
    const int64_t n = blk_ptr[b + 1] - blk_ptr[b];
    double* o = out + out_ptr[b];
    std::fill(o, o + n * n, 0.0);
    for (int64_t i = 0; i < n; ++i) {
      const int64_t r = dofs[i] / d, rc = dofs[i] % d;
      for (int64_t p = rowptr[r]; p < rowptr[r + 1]; ++p) {
        const int64_t c0 = (int64_t)colidx[p] * d;
        // dofs are sorted ascending: locate the first dof >= c0
        const int32_t* q = std::lower_bound(dofs, dofs + n, (int32_t)c0);
        for (; q < dofs + n && *q < c0 + d; ++q) o[i * n + (q - dofs)] = vals[p * d * d + rc * d + (*q - c0)];
      }
    }
  }
  return 0;
}

int alfi_host_num_threads() { return omp_get_max_threads(); }
// launchers such as torch.distributed.run export OMP_NUM_THREADS=1; the generator's own thread count is set explicitly
int alfi_host_set_num_threads(int n) {
  if (n > 0) omp_set_num_threads(n);
  return omp_get_max_threads();
}


// ---------------------------------------------------------------------------------------------------------------------
// SUPG and GLS stabilisation of the momentum equation (alfi/stabilisation.py:47-97 with the Shakib-Hughes-Johan coefficient,
// alfi/solver.py:204-234, state = u, body force f):
//   Lu   = -nu div(2 sym grad u) + (grad u) u - f   (+ grad p, zero for the piecewise constant pressure)
//   beta = (4 u.u / h^2 + magic (4 nu / h^2)^2)^(-1/2)
//   SUPG: weight * beta * inner(Lu, dot(grad(v), u)) * dx(degree = 2k)
//   GLS:  weight * beta * inner(Lu, L_w v) * dx(degree = 2k),  L_w v = -nu div(2 sym grad v) + (grad v) w,
//         w = the velocity at the start of the solve (z_last, solver.py:199, 205, 215), not differentiated
// by quadrature (beta is not polynomial).  F (n dofs, may be NULL) += the residual contribution; vals (BSR, may be NULL)
// += its Newton linearisation about u.  The test side of basis pair (a, i) is the d-vector T_aik:
//   SUPG: T_aik = delta_ik s_a,   GLS: T_aik = delta_ik (sw_a - nu Lap phi_a) - nu d_k d_i phi_a,
//   s_a = u.grad phi_a,  sw_a = w.grad phi_a;
//   F[a,i]        += wgt beta sum_k Lu_k T_aik,
//   dF[a,i; b,j]  += wgt sum_k T_aik (dbeta_j Lu_k + beta (dLu)_kj)   (+ SUPG: wgt beta Lu_i phi_b d_j phi_a),
//   dbeta_j = -4 beta^3 u_j phi_b / h^2,
//   (dLu)_kj = -nu (delta_kj Lap phi_b + d_k d_j phi_b) + delta_kj s_b + phi_b d_j u_k.
// phi (nq, nloc), dphi (nq, nloc, d+1), d2phi (nq, nloc, d+1, d+1): basis and its derivatives w.r.t. the barycentric
// coordinates at the quadrature points; wq (nq) sums to 1; h (ncell): cell size; U (nnode, d): state; W (nnode, d): the GLS
// wind; fq (ncell, nq, d, may be NULL): the body force at the quadrature points.
// ---------------------------------------------------------------------------------------------------------------------
static int host_stabilisation(bool gls, int64_t ncell, int nloc, int d, const int32_t* cell_nodes, const double* g,
                              const double* vol, const double* h, int nq, const double* wq, const double* phi,
                              const double* dphi, const double* d2phi, const double* U, const double* W, const double* fq,
                              double nu, double weight, double magic, const int32_t* rowptr, const int32_t* colidx,
                              double* vals, double* F) {
  const int nv = d + 1;
  const int ndof = nloc * d;
  int err = 0;
#pragma omp parallel
  {
    std::vector<double> Ae((size_t)ndof * ndof), Fe(ndof), Uk((size_t)nloc * d), Wk((size_t)nloc * d), gp((size_t)nloc * d),
        hs((size_t)nloc * d * d), lap(nloc), s(nloc), tq(nloc), C((size_t)d * ndof);
#pragma omp for schedule(dynamic, 64)
    for (int64_t c = 0; c < ncell; ++c) {
      const int32_t* cn = cell_nodes + c * nloc;
      const double* gc = g + c * nv * d;
      for (int a = 0; a < nloc; ++a)
        for (int x = 0; x < d; ++x) {
          Uk[a * d + x] = U[(int64_t)cn[a] * d + x];
          if (gls) Wk[a * d + x] = W[(int64_t)cn[a] * d + x];
        }
      std::fill(Ae.begin(), Ae.end(), 0.0);
      std::fill(Fe.begin(), Fe.end(), 0.0);
      const double h2 = h[c] * h[c];
      for (int q = 0; q < nq; ++q) {
        const double* ph = phi + (size_t)q * nloc;
        // physical gradients and Hessians of the basis at this point
        for (int a = 0; a < nloc; ++a) {
          const double* da = dphi + ((size_t)q * nloc + a) * nv;
          const double* ha = d2phi + ((size_t)q * nloc + a) * nv * nv;
          for (int x = 0; x < d; ++x) {
            double t = 0.0;
            for (int i = 0; i < nv; ++i) t += da[i] * gc[i * d + x];
            gp[a * d + x] = t;
          }
          double l = 0.0;
          for (int x = 0; x < d; ++x)
            for (int y = 0; y < d; ++y) {
              double t = 0.0;
              for (int i = 0; i < nv; ++i)
                for (int k = 0; k < nv; ++k) t += ha[i * nv + k] * gc[i * d + x] * gc[k * d + y];
              hs[((size_t)a * d + x) * d + y] = t;
              if (x == y) l += t;
            }
          lap[a] = l;
        }
        // state (and wind) at the point
        double u[3] = {0, 0, 0}, w[3] = {0, 0, 0}, Gu[3][3] = {{0}}, Lu[3] = {0, 0, 0};
        for (int a = 0; a < nloc; ++a)
          for (int i = 0; i < d; ++i) {
            const double ui = Uk[a * d + i];
            u[i] += ph[a] * ui;
            if (gls) w[i] += ph[a] * Wk[a * d + i];
            for (int x = 0; x < d; ++x) Gu[i][x] += gp[a * d + x] * ui;
            Lu[i] -= nu * lap[a] * ui;                                             // -nu Lap u_i
            for (int j = 0; j < d; ++j) Lu[j] -= nu * hs[((size_t)a * d + j) * d + i] * ui;   // -nu d_j div u
          }
        for (int i = 0; i < d; ++i)
          for (int x = 0; x < d; ++x) Lu[i] += u[x] * Gu[i][x];
        if (fq)
          for (int i = 0; i < d; ++i) Lu[i] -= fq[((size_t)c * nq + q) * d + i];
        double uu = 0.0;
        for (int i = 0; i < d; ++i) uu += u[i] * u[i];
        const double vis = 4.0 * nu / h2;
        const double beta = 1.0 / std::sqrt(4.0 * uu / h2 + magic * vis * vis);
        // s_a = u.grad phi_a; tq_a = the diagonal part of the test side (SUPG: s_a, GLS: w.grad phi_a - nu Lap phi_a)
        for (int a = 0; a < nloc; ++a) {
          double t = 0.0, tw = 0.0;
          for (int x = 0; x < d; ++x) {
            t += u[x] * gp[a * d + x];
            tw += w[x] * gp[a * d + x];
          }
          s[a] = t;
          tq[a] = gls ? tw - nu * lap[a] : t;
        }
        const double wt = wq[q] * vol[c] * weight;
        if (!gls) {
          // (SUPG keeps the association of its first host pass: with fq = NULL the result is the same to the bit)
          for (int a = 0; a < nloc; ++a)
            for (int i = 0; i < d; ++i) Fe[a * d + i] += wt * beta * Lu[i] * s[a];
        } else {
          for (int a = 0; a < nloc; ++a)
            for (int i = 0; i < d; ++i) {
              double t = Lu[i] * tq[a];
              for (int k = 0; k < d; ++k) t -= nu * Lu[k] * hs[((size_t)a * d + k) * d + i];
              Fe[a * d + i] += wt * beta * t;
            }
        }
        if (vals && !gls) {
          const double b3 = -4.0 * beta * beta * beta / h2;
          for (int a = 0; a < nloc; ++a)
            for (int i = 0; i < d; ++i) {
              double* row = Ae.data() + (size_t)(a * d + i) * ndof;
              for (int b = 0; b < nloc; ++b)
                for (int j = 0; j < d; ++j) {
                  double dL = -nu * hs[((size_t)b * d + i) * d + j] + ph[b] * Gu[i][j];
                  if (i == j) dL += -nu * lap[b] + s[b];
                  row[b * d + j] += wt * (b3 * u[j] * ph[b] * Lu[i] * s[a] + beta * dL * s[a] +
                                          beta * Lu[i] * ph[b] * gp[a * d + j]);
                }
            }
        } else if (vals) {
          const double b3 = -4.0 * beta * beta * beta / h2;
          // GLS: C[k][(b, j)] = wt (b3 u_j phi_b Lu_k + beta (dLu)_kj), row (a, i) = sum_k T_aik C[k]
          for (int k = 0; k < d; ++k)
            for (int b = 0; b < nloc; ++b)
              for (int j = 0; j < d; ++j) {
                double dL = -nu * hs[((size_t)b * d + k) * d + j] + ph[b] * Gu[k][j];
                if (k == j) dL += -nu * lap[b] + s[b];
                C[(size_t)k * ndof + b * d + j] = wt * (b3 * u[j] * ph[b] * Lu[k] + beta * dL);
              }
          for (int a = 0; a < nloc; ++a)
            for (int i = 0; i < d; ++i) {
              double* row = Ae.data() + (size_t)(a * d + i) * ndof;
              const double* Ci = C.data() + (size_t)i * ndof;
              for (int bj = 0; bj < ndof; ++bj) row[bj] += tq[a] * Ci[bj];
              for (int k = 0; k < d; ++k) {
                const double hk = -nu * hs[((size_t)a * d + k) * d + i];
                const double* Ck = C.data() + (size_t)k * ndof;
                for (int bj = 0; bj < ndof; ++bj) row[bj] += hk * Ck[bj];
              }
            }
        }
      }
      if (F)
        for (int a = 0; a < nloc; ++a)
          for (int i = 0; i < d; ++i) {
#pragma omp atomic
            F[(int64_t)cn[a] * d + i] += Fe[a * d + i];
          }
      if (vals)
        for (int a = 0; a < nloc; ++a) {
          const int64_t lo = rowptr[cn[a]], hi = rowptr[cn[a] + 1];
          for (int b = 0; b < nloc; ++b) {
            const int64_t pos = find_col(colidx, lo, hi, cn[b]);
            if (pos >= hi || colidx[pos] != cn[b]) {
              err = 1;
              continue;
            }
            double* dst = vals + pos * d * d;
            for (int cc = 0; cc < d; ++cc)
              for (int dd = 0; dd < d; ++dd) {
#pragma omp atomic
                dst[cc * d + dd] += Ae[(size_t)(a * d + cc) * ndof + b * d + dd];
              }
          }
        }
    }
  }
  return err ? -2 : 0;
}

int alfi_host_supg(int64_t ncell, int nloc, int d, const int32_t* cell_nodes, const double* g, const double* vol,
                   const double* h, int nq, const double* wq, const double* phi, const double* dphi, const double* d2phi,
                   const double* U, double nu, double weight, double magic, const int32_t* rowptr, const int32_t* colidx,
                   double* vals, double* F, const double* fq) {
  return host_stabilisation(false, ncell, nloc, d, cell_nodes, g, vol, h, nq, wq, phi, dphi, d2phi, U, nullptr, fq, nu, weight,
                            magic, rowptr, colidx, vals, F);
}

int alfi_host_gls(int64_t ncell, int nloc, int d, const int32_t* cell_nodes, const double* g, const double* vol,
                  const double* h, int nq, const double* wq, const double* phi, const double* dphi, const double* d2phi,
                  const double* U, const double* W, double nu, double weight, double magic, const int32_t* rowptr,
                  const int32_t* colidx, double* vals, double* F, const double* fq) {
  if (!W) return -1;
  return host_stabilisation(true, ncell, nloc, d, cell_nodes, g, vol, h, nq, wq, phi, dphi, d2phi, U, W, fq, nu, weight, magic,
                            rowptr, colidx, vals, F);
}

// ---------------------------------------------------------------------------------------------------------------------
// Burman interior-penalty stabilisation of the Scott-Vogelius pair (alfi/stabilisation.py:139-162, alfi/solver.py:226-234;
// alfi_amd/burman.py states the form and its linearisation).  Per interior facet f (tables of burman.FacetTable):
//   union (nf, nu): K+'s nodes, then K-'s nodes off F;  J (nf, nqs, nu): jumps of the normal derivatives at the points of the
//   exact rule (weights ws, summing to 1);  area, coef (nf): |F| and 0.5 avg(h)^2;  cfg (nf): K+'s configuration, phin
//   (ncfg, nqn, nloc): K+'s basis at the nonlinear rule's points (weights wn), zero off F.
// Pass 1 (a facet each): beta = sum_q wn u.u-root, m[b][j] = sum_q wn phi_b u_j / root, jq[q][i] = jump of d_n u_i at point q.
// Pass 2 (a BSR block each, vals may be NULL): the contributors (facet, a * nu + b) of the block in list order,
//   block += weight coef (beta S_ab I + g_a (x) m_b),  S_ab = |F| sum_q ws J_qa J_qb,  g_a = |F| sum_q ws J_qa jq_q.
// beta_out (nf, may be NULL): beta_F of every facet.
// Pass 3 (a node each, F may be NULL): the contributors (facet, a) of the node, F[node] += weight coef beta g_a.
// Every entry is summed by one thread in a fixed order: the result does not depend on the number of threads.
// ---------------------------------------------------------------------------------------------------------------------
int alfi_host_burman(int64_t nf, int nu, int nloc, int d, int nqs, int nqn, const int32_t* unodes, const int32_t* cfg,
                     const double* J, const double* area, const double* coef, const double* ws, const double* wn,
                     const double* phin, const double* U, double weight, int64_t nnzb, const int64_t* bptr,
                     const int32_t* bfac, const uint16_t* bab, double* vals, int64_t nnode, const int64_t* nptr,
                     const int32_t* nfac, const uint16_t* na, double* F, double* beta_out) {
  if (d < 2 || d > 3 || nqs > 64 || nqn > 64 || nloc > 64) return -1;
  const int rec = 1 + nqs * d + nloc * d;      // beta | jq (nqs, d) | m (nloc, d)
  std::vector<double> R((size_t)std::max<int64_t>(nf, 1) * rec);
#pragma omp parallel for schedule(static)
  for (int64_t f = 0; f < nf; ++f) {
    const int32_t* un = unodes + f * nu;
    const double* ph = phin + (size_t)cfg[f] * nqn * nloc;
    double* r = R.data() + (size_t)f * rec;
    double beta = 0.0;
    double* m = r + 1 + nqs * d;
    for (int t = 0; t < nloc * d; ++t) m[t] = 0.0;
    for (int q = 0; q < nqn; ++q) {
      double u[3] = {0.0, 0.0, 0.0};
      for (int a = 0; a < nloc; ++a)
        for (int i = 0; i < d; ++i) u[i] += ph[q * nloc + a] * U[(int64_t)un[a] * d + i];
      double uu = 1e-10;
      for (int i = 0; i < d; ++i) uu += u[i] * u[i];
      const double root = std::sqrt(uu);
      beta += wn[q] * root;
      for (int a = 0; a < nloc; ++a)
        for (int i = 0; i < d; ++i) m[a * d + i] += wn[q] * ph[q * nloc + a] * u[i] / root;
    }
    r[0] = beta;
    if (beta_out) beta_out[f] = beta;
    const double* Jf = J + (size_t)f * nqs * nu;
    for (int q = 0; q < nqs; ++q)
      for (int i = 0; i < d; ++i) {
        double t = 0.0;
        for (int a = 0; a < nu; ++a) t += Jf[q * nu + a] * U[(int64_t)un[a] * d + i];
        r[1 + q * d + i] = t;
      }
  }
  if (vals) {
#pragma omp parallel for schedule(dynamic, 1024)
    for (int64_t k = 0; k < nnzb; ++k) {
      double acc[9] = {0.0};
      for (int64_t p = bptr[k]; p < bptr[k + 1]; ++p) {
        const int64_t f = bfac[p];
        const int a = bab[p] / nu, b = bab[p] % nu;
        const double* Jf = J + (size_t)f * nqs * nu;
        const double* r = R.data() + (size_t)f * rec;
        double s = 0.0, g[3] = {0.0, 0.0, 0.0};
        for (int q = 0; q < nqs; ++q) {
          const double wa = ws[q] * Jf[q * nu + a];
          s += wa * Jf[q * nu + b];
          for (int i = 0; i < d; ++i) g[i] += wa * r[1 + q * d + i];
        }
        const double c = weight * coef[f], A = area[f];
        for (int i = 0; i < d; ++i) {
          acc[i * d + i] += c * r[0] * A * s;
          if (b < nloc)
            for (int j = 0; j < d; ++j) acc[i * d + j] += c * A * g[i] * r[1 + nqs * d + b * d + j];
        }
      }
      for (int t = 0; t < d * d; ++t) vals[k * d * d + t] += acc[t];
    }
  }
  if (F) {
#pragma omp parallel for schedule(dynamic, 1024)
    for (int64_t n = 0; n < nnode; ++n) {
      double acc[3] = {0.0, 0.0, 0.0};
      for (int64_t p = nptr[n]; p < nptr[n + 1]; ++p) {
        const int64_t f = nfac[p];
        const int a = na[p];
        const double* Jf = J + (size_t)f * nqs * nu;
        const double* r = R.data() + (size_t)f * rec;
        const double c = weight * coef[f] * r[0] * area[f];
        for (int q = 0; q < nqs; ++q) {
          const double wa = ws[q] * Jf[q * nu + a];
          for (int i = 0; i < d; ++i) acc[i] += c * wa * r[1 + q * d + i];
        }
      }
      for (int i = 0; i < d; ++i) F[n * d + i] += acc[i];
    }
  }
  return 0;
}

// The group finder of libalfi_hip.so's alfi_patches_find_groups (find_groups.h) on host arrays: the CPU leg of its tests.
// Returns the number of patches that got groups.
int64_t alfi_host_find_groups(int bs, int64_t nbrows, int64_t npatch, const int64_t* patch_ptr, const int32_t* patch_dofs,
                              const int32_t* rowptr, const int32_t* colidx, int32_t* group_out) {
  return alfi_find_groups_host(bs, nbrows, npatch, patch_ptr, patch_dofs, rowptr, colidx, group_out);
}

}  // extern "C"

// The planners of alfi_patches_set / _set_groups / _set_multiplicative (patch_plan.h) on host arrays: the CPU leg of their
// tests.  Each returns a handle (never NULL); alfi_host_plan_status gives the planner's code and message, alfi_host_plan_table
// enumerates what it built, alfi_host_plan_free releases it.
struct alfi_host_plan {
  PatchLayout lay;
  CondPlan cond;
  SweepPlan sweep;
  SweepCondPlan swc;
  std::vector<int64_t> f32_ptr, ranges;
  int rc = 0;
  std::string err;
  struct Entry {
    const char* name;
    const void* ptr;
    int64_t count;   // -1: a scalar (one int64, kept in value)
    int item;
    int64_t value;
  };
  std::vector<Entry> tab;
  template <class T>
  void table(const char* name, const std::vector<T>& v) { tab.push_back({name, v.data(), (int64_t)v.size(), (int)sizeof(T), 0}); }
  void scalar(const char* name, int64_t v) { tab.push_back({name, nullptr, -1, 8, v}); }
};
#define ALFI_PLAN_TABLE(s, f) h->table(#f, h->s.f)
#define ALFI_PLAN_SCALAR(s, f) h->scalar(#f, (int64_t)h->s.f)

// alfi_host_plan_f32_layout and alfi_host_plan_macro_f32_layout: patches of up to max_np dofs
static alfi_host_plan* plan_f32_layout(int64_t npatch, const int64_t* patch_ptr, int max_np, const char* what) {
  alfi_host_plan* h = new alfi_host_plan();
  for (int64_t p = 0; p < npatch; ++p)
    if (patch_ptr[p + 1] - patch_ptr[p] <= 0 || patch_ptr[p + 1] - patch_ptr[p] > max_np) {
      h->rc = plan_fail(&h->err, "patch %lld has %lld dofs; %s holds patches of 1..%d", (long long)p,
                        (long long)(patch_ptr[p + 1] - patch_ptr[p]), what, max_np);
      return h;
    }
  const int64_t total = plan_f32_offsets(npatch, patch_ptr, &h->f32_ptr);
  h->table("f32_ptr", h->f32_ptr);
  h->scalar("inv32_floats", total);
  h->scalar("rows_per_load", F32_ROWS);
  h->scalar("align_floats", F32_ALIGN);
  return h;
}

extern "C" {

alfi_host_plan* alfi_host_plan_patch_layout(int64_t n, int64_t npatch, const int64_t* patch_ptr, const int32_t* patch_dofs) {
  alfi_host_plan* h = new alfi_host_plan();
  h->rc = plan_patch_layout(n, npatch, patch_ptr, patch_dofs, PATCH_MAX, &h->lay, &h->err);
  if (h->rc != 0) return h;
  ALFI_PLAN_TABLE(lay, inv_ptr); ALFI_PLAN_TABLE(lay, stage_ptr); ALFI_PLAN_TABLE(lay, dof_ptr); ALFI_PLAN_TABLE(lay, dof_pos);
  ALFI_PLAN_SCALAR(lay, sum_n); ALFI_PLAN_SCALAR(lay, sum_n2); ALFI_PLAN_SCALAR(lay, inv_doubles);
  ALFI_PLAN_SCALAR(lay, stage_len); ALFI_PLAN_SCALAR(lay, max_np);
  return h;
}

// the single-precision storage of a level's dense inverses (patch_plan.h): the offsets of the patches (floats, npatch + 1) and
// the scalars of the layout
alfi_host_plan* alfi_host_plan_f32_layout(int64_t npatch, const int64_t* patch_ptr) {
  return plan_f32_layout(npatch, patch_ptr, SMALL_PATCH_MAX, "FP32 storage");
}
// the same for the levels of alfi_patches_set_macro_storage: patches of up to PATCH_MAX dofs
alfi_host_plan* alfi_host_plan_macro_f32_layout(int64_t npatch, const int64_t* patch_ptr) {
  return plan_f32_layout(npatch, patch_ptr, PATCH_MAX, "FP32 macro-star storage");
}
// the ranges an FP32 level of big patches is factored in (patch_plan.h: plan_f32_ranges): inv_ptr as plan_patch_layout returns
// it, the cap in doubles
alfi_host_plan* alfi_host_plan_f32_ranges(int64_t npatch, const int64_t* inv_ptr, int64_t cap_doubles) {
  alfi_host_plan* h = new alfi_host_plan();
  const int64_t work = plan_f32_ranges(npatch, inv_ptr, cap_doubles, &h->ranges);
  h->table("ranges", h->ranges);
  h->scalar("work_doubles", work);
  return h;
}
// all offsets of an n x n inverse at once: out[r * n + c] = f32_inv_index(r, c, n), r < f32_ld(n) (big patches: 16 M entries)
void alfi_host_f32_index_table(int n, int64_t* out) {
  const int ld = f32_ld(n);
  for (int r = 0; r < ld; ++r)
    for (int c = 0; c < n; ++c) out[(int64_t)r * n + c] = f32_inv_index(r, c, n);
}
// the row-piece storage itself and its FP64 wrapper: out[r * n + c] = piece_index(r, c, n, ld, min_rows) / patch_inv_index(r, c, n,
// ld), r < ld
void alfi_host_piece_index_table(int n, int ld, int min_rows, int64_t* out) {
  for (int r = 0; r < ld; ++r)
    for (int c = 0; c < n; ++c) out[(int64_t)r * n + c] = piece_index(r, c, n, ld, min_rows);
}
void alfi_host_patch_index_table(int n, int ld, int64_t* out) {
  for (int r = 0; r < ld; ++r)
    for (int c = 0; c < n; ++c) out[(int64_t)r * n + c] = patch_inv_index(r, c, n, ld);
}
// entry (r, c) of an n x n inverse in that storage, r < alfi_host_f32_ld(n) (pad rows included), c < n; floats a patch occupies
int64_t alfi_host_f32_index(int r, int c, int n) { return f32_inv_index(r, c, n); }
int alfi_host_f32_ld(int n) { return f32_ld(n); }
int64_t alfi_host_f32_patch_floats(int n) { return f32_patch_floats(n); }

alfi_host_plan* alfi_host_plan_condensed(int bs, int64_t nbrows, int64_t npatch, const int64_t* patch_ptr, const int32_t* patch_dofs,
                                         const int32_t* group, const int32_t* rowptr, const int32_t* colidx) {
  alfi_host_plan* h = new alfi_host_plan();
  h->rc = plan_condensed(bs, nbrows, npatch, patch_ptr, patch_dofs, group, rowptr, colidx, COND_SIGMA_ROWS, &h->cond, &h->err);
  if (h->rc != 0) return h;
  ALFI_PLAN_TABLE(cond, dofs); ALFI_PLAN_TABLE(cond, slot); ALFI_PLAN_TABLE(cond, gptr); ALFI_PLAN_TABLE(cond, g_off);
  ALFI_PLAN_TABLE(cond, g_m); ALFI_PLAN_TABLE(cond, g_sc); ALFI_PLAN_TABLE(cond, g_uoff); ALFI_PLAN_TABLE(cond, g_mat);
  ALFI_PLAN_TABLE(cond, g_sidx); ALFI_PLAN_TABLE(cond, sidx); ALFI_PLAN_TABLE(cond, p_nI); ALFI_PLAN_TABLE(cond, sptr);
  ALFI_PLAN_TABLE(cond, sinv_ptr); ALFI_PLAN_TABLE(cond, s_uptr); ALFI_PLAN_TABLE(cond, s_uidx); ALFI_PLAN_TABLE(cond, order);
  ALFI_PLAN_TABLE(cond, chptr); ALFI_PLAN_TABLE(cond, ch_patch); ALFI_PLAN_TABLE(cond, ch_row); ALFI_PLAN_TABLE(cond, uptr);
  ALFI_PLAN_TABLE(cond, u_dst); ALFI_PLAN_TABLE(cond, xp_ptr); ALFI_PLAN_TABLE(cond, xp_grp); ALFI_PLAN_TABLE(cond, g_xp);
  ALFI_PLAN_TABLE(cond, bp_ptr); ALFI_PLAN_TABLE(cond, bp_grp); ALFI_PLAN_TABLE(cond, g_bp); ALFI_PLAN_TABLE(cond, gcptr);
  ALFI_PLAN_TABLE(cond, gc);
  ALFI_PLAN_SCALAR(cond, ngroups); ALFI_PLAN_SCALAR(cond, mat_doubles); ALFI_PLAN_SCALAR(cond, sinv_doubles);
  ALFI_PLAN_SCALAR(cond, lds_bytes); ALFI_PLAN_SCALAR(cond, lds_front);
  ALFI_PLAN_SCALAR(cond, lds_back); ALFI_PLAN_SCALAR(cond, lds_gfront); ALFI_PLAN_SCALAR(cond, lds_gback);
  ALFI_PLAN_SCALAR(cond, max_s); ALFI_PLAN_SCALAR(cond, max_m); ALFI_PLAN_SCALAR(cond, max_pairs); ALFI_PLAN_SCALAR(cond, umax);
  return h;
}

alfi_host_plan* alfi_host_plan_sweep(int bs, int64_t nbrows, int64_t npatch, const int64_t* patch_ptr, const int32_t* patch_dofs,
                                     const int32_t* rowptr, const int32_t* colidx, int64_t nit, const int64_t* iterset,
                                     int symmetrise) {
  alfi_host_plan* h = new alfi_host_plan();
  bool big = false;
  h->rc = check_sweep(bs, npatch, patch_ptr, patch_dofs, SMALL_PATCH_MAX, nit, iterset, &big, &h->err);
  if (h->rc == 0)
    h->rc = plan_sweep(bs, nbrows, npatch, patch_ptr, patch_dofs, rowptr, colidx, nit, iterset, symmetrise != 0, big, &h->sweep,
                       &h->err);
  if (h->rc != 0) return h;
  ALFI_PLAN_TABLE(sweep, seq); ALFI_PLAN_TABLE(sweep, wave_ptr); ALFI_PLAN_TABLE(sweep, items); ALFI_PLAN_TABLE(sweep, pred0);
  ALFI_PLAN_TABLE(sweep, succ_ptr); ALFI_PLAN_TABLE(sweep, succ); ALFI_PLAN_TABLE(sweep, rowtab);
  ALFI_PLAN_SCALAR(sweep, big); ALFI_PLAN_SCALAR(sweep, nitems);
  return h;
}

// the work lists of a sweep over condensed patches (patch_plan.h: plan_sweep_condensed): seq / wave_ptr as alfi_host_plan_sweep
// returns them, gcptr / chptr as alfi_host_plan_condensed does
alfi_host_plan* alfi_host_plan_sweep_condensed(int bs, int64_t npatch, const int64_t* patch_ptr, const int32_t* patch_dofs,
                                               int64_t nwave, const int64_t* wave_ptr, const int32_t* seq, const int64_t* gcptr,
                                               const int64_t* chptr) {
  alfi_host_plan* h = new alfi_host_plan();
  h->rc = plan_sweep_condensed(bs, npatch, patch_ptr, patch_dofs, nwave, wave_ptr, seq, gcptr, chptr, &h->swc, &h->err);
  if (h->rc != 0) return h;
  ALFI_PLAN_TABLE(swc, wk_ptr); ALFI_PLAN_TABLE(swc, wc_ptr); ALFI_PLAN_TABLE(swc, wn_ptr); ALFI_PLAN_TABLE(swc, gchunk);
  ALFI_PLAN_TABLE(swc, schunk); ALFI_PLAN_TABLE(swc, node);
  return h;
}
#undef ALFI_PLAN_TABLE
#undef ALFI_PLAN_SCALAR

int alfi_host_plan_status(const alfi_host_plan* h, const char** message) {
  if (message) *message = h->err.c_str();
  return h->rc;
}

// table i of the plan: 0, or -1 past the last one
int alfi_host_plan_table(const alfi_host_plan* h, int64_t i, const char** name, const void** ptr, int64_t* count, int* item_size) {
  if (i < 0 || i >= (int64_t)h->tab.size()) return -1;
  const alfi_host_plan::Entry& e = h->tab[(size_t)i];
  *name = e.name; *ptr = e.count < 0 ? &e.value : e.ptr; *count = e.count; *item_size = e.item;
  return 0;
}

void alfi_host_plan_free(alfi_host_plan* h) { delete h; }

}  // extern "C"
