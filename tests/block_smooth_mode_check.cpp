// The dispatch rule of the block smoother and the sizing of its partial buffers (alfi_amd/csrc/block_cols.h: block_smooth_mode,
// block_partial_per_slot, block_dot_vectors, block_slots_needed, block_piece) under host sanitizers: a stand-alone program.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan
//       -I alfi_amd/csrc tests/block_smooth_mode_check.cpp
// Prints "OK <checks>" and exits 0, or says what failed and exits 1.
#include <cstdio>
#include <vector>
#include "block_cols.h"

static int checks = 0, failed = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    ++checks;                                                            \
    if (!(cond)) {                                                       \
      ++failed;                                                          \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);              \
    }                                                                    \
  } while (0)

static BlockSmoothFacts facts(bool kernels, bool fused, bool part, bool fi, bool il, int waves, int width) {
  BlockSmoothFacts f;
  f.block_kernels = kernels;
  f.block_fused = fused;
  f.partitioned = part;
  f.fused_iteration = fi;
  f.applies_il = il;
  f.apply_waves = waves;
  f.piece_width = width;
  return f;
}

int main() {
  // every combination of the facts against the rule written out the long way
  const int waves[] = {0, 1, 4, 8}, widths[] = {0, 1, 2, 3, 4};
  for (int m = 0; m < 32; ++m)
    for (int w : waves)
      for (int pw : widths) {
        const bool kernels = m & 1, fused = m & 2, part = m & 4, fi = m & 8, il = m & 16;
        int want;
        if (!kernels || part) want = 0;
        else if (!fi) want = 1;
        else if (!fused) want = 0;
        else want = (il || w != 0 || pw >= 2) ? 2 : 0;
        CHECK(block_smooth_mode(facts(kernels, fused, part, fi, il, w, pw)) == want);
      }
  CHECK(BLOCK_SMOOTH_LOOP == 0 && BLOCK_SMOOTH_LOCKSTEP == 1 && BLOCK_SMOOTH_FUSED == 2);
  // the cases the text names
  CHECK(block_smooth_mode(facts(true, true, false, true, true, 0, 0)) == 2);      // interleaved copy
  CHECK(block_smooth_mode(facts(true, true, false, true, false, 4, 0)) == 2);     // dense stars
  CHECK(block_smooth_mode(facts(true, true, false, true, false, 0, 3)) == 2);     // pieces of three
  CHECK(block_smooth_mode(facts(true, true, false, true, false, 0, 0)) == 0);     // chunked condensed form, few macro stars
  CHECK(block_smooth_mode(facts(true, true, false, true, false, 0, 1)) == 0);
  CHECK(block_smooth_mode(facts(true, false, false, true, true, 0, 0)) == 0);     // the switch: the parent's path
  CHECK(block_smooth_mode(facts(true, false, false, false, true, 0, 0)) == 1);    // ... which leaves lockstep alone
  CHECK(block_smooth_mode(facts(false, true, false, false, true, 4, 4)) == 0);
  CHECK(block_smooth_mode(facts(true, true, true, true, true, 4, 4)) == 0);

  // partial buffers: two sets per slot, each a whole [red_blocks][red_maxv] table; a real allocation of every size the
  // workspace can have is written at the last entry of every slot's two sets
  CHECK(block_partial_set(1024, 32) == 32768 && block_partial_per_slot(1024, 32) == 65536);
  CHECK(block_partial_per_slot(1, 1) == 2 && block_partial_per_slot(0, 32) == 0);
  for (int have = 0; have <= BLOCK_NV; ++have)
    for (int ncol = 1; ncol <= 9; ++ncol) {
      const int slots = block_slots_needed(have, ncol);
      CHECK(slots >= have && slots <= BLOCK_NV && slots >= (ncol < BLOCK_NV ? ncol : BLOCK_NV));
      const int64_t per = block_partial_per_slot(1024, 32), set = block_partial_set(1024, 32);
      std::vector<double> buf((size_t)(slots * per), 0.0);
      for (int s = 0; s < slots; ++s) {
        buf[(size_t)(s * per + 1023 * 32 + 31)] = 1.0;            // last partial of the first set
        buf[(size_t)(s * per + set + 1023 * 32 + 31)] = 2.0;      // ... of the second
      }
      double sum = 0.0;
      for (double v : buf) sum += v;
      CHECK(sum == 3.0 * slots);
    }

  // dot vectors of an instantiation: j + 1 rounded up, never below it, never above 16
  for (int nv = -1; nv <= 18; ++nv) {
    const int r = block_dot_vectors(nv);
    if (nv < 1 || nv > 16) CHECK(r == 0);
    else CHECK(r >= nv && (r == 4 || r == 8 || r == 16) && (r == 4 || r / 2 < nv));
  }

  // the pieces of a chunk of slots: consecutive slots, at most one piece of one column, every slot exactly once
  for (int n = 2; n <= BLOCK_NV; ++n)
    for (int width = 2; width <= BLOCK_NV; ++width) {
      const BlockCols slots = block_chunk(n, nullptr, 0);
      int seen[BLOCK_NV] = {0, 0, 0, 0}, singles = 0;
      for (int q = 0; q < block_pieces(n, width); ++q) {
        const BlockCols p = block_piece(slots, width, q);
        CHECK(p.n >= 1 && p.n <= width);
        singles += p.n == 1;
        for (int i = 0; i < p.n; ++i) {
          CHECK(p.c[i] == p.c[0] + i && p.c[i] < n);
          ++seen[p.c[i]];
        }
      }
      CHECK(singles <= 1);
      for (int s = 0; s < n; ++s) CHECK(seen[s] == 1);
    }

  if (failed) {
    std::printf("%d of %d checks failed\n", failed, checks);
    return 1;
  }
  std::printf("OK %d\n", checks);
  return 0;
}
