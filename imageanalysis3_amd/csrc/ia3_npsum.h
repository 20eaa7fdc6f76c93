// NumPy's summation order for np.sum / np.add.reduce over a contiguous axis of n <= 512 floating-point elements
// (numpy/_core/src/umath/loops_utils.h.src, pairwise sum): the one statement of it in this library.
//   n < 8            one accumulator, left to right;
//   8 <= n <= 128    eight accumulators r[j] = a[j], r[j] += a[i + j] for i = 8, 16, ... while a whole group of eight
//                    is left, combined as ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), then the up to seven
//                    leftover elements added left to right;
//   n > 128          the sum of the first n/2 rounded down to a multiple of eight plus the sum of the rest, each by
//                    the same rule (n <= 512: at most three such splits deep, unrolled below instead of a recursion).
// The reduction starts from the ufunc's identity, so the whole range goes through this rule (NumPy 2.2; checked for
// every n from 1 to 512 by tests/test_fastfit_cpu.py).  `at(i)` yields element i already in the accumulation type T:
// callers form products on the fly (fastfit.hip) or read an array (ia3_init.h).  Additions only: nothing here can be
// contracted into a fused multiply-add.
#pragma once
#include "ia3_model.h"

namespace ia3 {

constexpr int NPSUM_BLOCK = 128, NPSUM_MAX = 512;

template <class T, class F>
IA3_HD T np_sum_block(F at, int off, int n) {   // n <= NPSUM_BLOCK
  if (n < 8) {
    T res = (T)0;
    for (int i = 0; i < n; ++i) res = res + at(off + i);
    return res;
  }
  T r[8];
  for (int j = 0; j < 8; ++j) r[j] = at(off + j);
  int i = 8;
  for (; i < n - (n % 8); i += 8)
    for (int j = 0; j < 8; ++j) r[j] = r[j] + at(off + i + j);
  T res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; ++i) res = res + at(off + i);
  return res;
}

// the splits, at most NPSUM_SPLITS deep: the larger part of n elements has at most n/2 + 8, so 512 -> 264 -> 140 -> 78
constexpr int NPSUM_SPLITS = 3;
template <class T, int D, class F>
IA3_HD T np_sum_split(F at, int off, int n) {
  if constexpr (D == 0) {
    return np_sum_block<T>(at, off, n);
  } else {
    if (n <= NPSUM_BLOCK) return np_sum_block<T>(at, off, n);
    int n2 = n / 2;
    n2 -= n2 % 8;
    const T a = np_sum_split<T, D - 1>(at, off, n2);
    const T b = np_sum_split<T, D - 1>(at, off + n2, n - n2);
    return a + b;
  }
}

// sum of at(0) .. at(n - 1), n <= NPSUM_MAX
template <class T, class F>
IA3_HD T np_sum_f(F at, int n) {
  return np_sum_split<T, NPSUM_SPLITS>(at, 0, n);
}

template <class T>
IA3_HD T np_sum(const T* a, int n) {
  return np_sum_f<T>([a](int i) { return a[i]; }, n);
}

}  // namespace ia3
