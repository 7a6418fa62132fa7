// Stand-alone check of the dispatch rule of the condensed apply's early-load form (csrc/cond_layout.h: cond_ahead,
// cond_ahead_front_waves) -- built and run by tests/test_cond_ahead_rule.py, once as the library has it and once with
// -DALFI_COND_AHEAD=0 (the A/B build: the rule is false everywhere).  Prints "OK <cases>" or the first mismatch.
#include <cstdio>

#include "cond_layout.h"

int main() {
  const int ms[] = {0, 1, 15, 16, 17, 45, 64};
  const int pairs[] = {0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1024, 5000};
  int cases = 0;
  for (int m : ms)
    for (int mp : pairs) {
      // long hand: groups of at most 16 entries, and no patch with more row pairs than the widest workgroup (8 waves) has lanes
      const bool want = ALFI_COND_AHEAD != 0 && m <= 16 && mp <= 512;
      if (cond_ahead(m, mp) != want) {
        std::printf("cond_ahead(%d, %d) = %d, expected %d\n", m, mp, (int)cond_ahead(m, mp), (int)want);
        return 1;
      }
      // where the rule holds a lane owns at most one row pair per phase
      if (cond_ahead(m, mp) && mp > 64 * cond_patch_waves(mp)) {
        std::printf("cond_ahead(%d, %d) with %d waves\n", m, mp, cond_patch_waves(mp));
        return 1;
      }
      ++cases;
    }
  // the front workgroup: whole waves of X pairs, then whole waves of B pairs; never more than twice the back kernel's waves
  const int xb[][3] = {{0, 0, 0}, {1, 0, 1}, {0, 1, 1}, {48, 84, 3}, {64, 64, 2}, {65, 64, 3}, {64, 65, 3}, {128, 128, 4},
                       {512, 128, 10}, {512, 512, 16}, {10, 6, 2}};
  for (const auto& c : xb) {
    if (cond_ahead_front_waves(c[0], c[1]) != c[2]) {
      std::printf("cond_ahead_front_waves(%d, %d) = %d, expected %d\n", c[0], c[1], cond_ahead_front_waves(c[0], c[1]), c[2]);
      return 1;
    }
    const int mp = c[0] > c[1] ? c[0] : c[1];
    if (mp <= 512 && cond_ahead_front_waves(c[0], c[1]) > 2 * cond_patch_waves(mp)) {
      std::printf("front waves of (%d, %d) above twice cond_patch_waves\n", c[0], c[1]);
      return 1;
    }
    ++cases;
  }
  if (COND_AHEAD_M != 16) {
    std::printf("COND_AHEAD_M = %d\n", COND_AHEAD_M);
    return 1;
  }
  std::printf("OK %d\n", cases);
  return 0;
}
