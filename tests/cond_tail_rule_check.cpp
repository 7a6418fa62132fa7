// Stand-alone check of the dispatch rule of the condensed apply's tail launch (csrc/cond_layout.h: cond_tail) -- built and run
// by tests/test_cond_tail_rule.py, once as the library has it and once with -DALFI_COND_TAIL=0 (the A/B build: the rule is
// false everywhere).  Prints "OK <cases>" or the first mismatch.
#include <cstdio>

#include "cond_layout.h"

int main() {
  const int xps[] = {0, 1, 48, 63, 64, 65, 128, 1000};
  const int scs[] = {0, 1, 8, 9, 27, 31, 32, 33, 45, 64};
  const int ss[] = {0, 1, 27, 62, 63, 64, 65, 66, 128, 585};
  int cases = 0;
  for (int xp : xps)
    for (int sc : scs)
      for (int s : ss) {
        // long hand: a quartet of the 256 lanes per row pair of X / W, four quarters of 8 columns of W, a skeleton that is one
        // chunk of 64 rows of the sigma launch
        const bool want = ALFI_COND_TAIL != 0 && xp <= 64 && sc <= 32 && s <= 64;
        if (cond_tail(xp, sc, s) != want) {
          std::printf("cond_tail(%d, %d, %d) = %d, expected %d\n", xp, sc, s, (int)cond_tail(xp, sc, s), (int)want);
          return 1;
        }
        ++cases;
      }
  // the bounds one at a time, the other two at theirs
  const int edge[][4] = {{64, 32, 64, 1}, {65, 32, 64, 0}, {64, 33, 64, 0}, {64, 32, 65, 0}, {48, 27, 63, 1}};
  for (const auto& e : edge) {
    if (cond_tail(e[0], e[1], e[2]) != (ALFI_COND_TAIL != 0 && e[3] != 0)) {
      std::printf("cond_tail(%d, %d, %d) = %d\n", e[0], e[1], e[2], (int)cond_tail(e[0], e[1], e[2]));
      return 1;
    }
    ++cases;
  }
  // where the rule holds a patch is one chunk of the sigma launch and a lane has at most one skeleton entry
  if (COND_TAIL_THREADS != 256 || COND_TAIL_QUARTER != 8 || COND_TAIL_S != 64 || COND_TAIL_S > COND_TAIL_THREADS) {
    std::printf("COND_TAIL_THREADS %d, COND_TAIL_QUARTER %d, COND_TAIL_S %d\n", COND_TAIL_THREADS, COND_TAIL_QUARTER, COND_TAIL_S);
    return 1;
  }
  if (ALFI_COND_TAIL != 0 && cond_tail(1, 1, COND_SIGMA_ROWS + 1)) {
    std::printf("cond_tail with a skeleton of two sigma chunks\n");
    return 1;
  }
  std::printf("OK %d\n", cases);
  return 0;
}
