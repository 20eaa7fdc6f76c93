// NumPy's summation order for np.sum / np.add.reduce over a contiguous axis of floating-point elements
// (numpy/_core/src/umath/loops_utils.h.src, pairwise sum): the one statement of it in this library.  np_sum_f covers
// n <= 512 with the splits unrolled; np_sum_any covers every n with the same block and the same split (np_sum_half), its
// recursion written as a loop over a small stack of pending parts.
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

// the first part of a split of n > NPSUM_BLOCK elements: n/2 rounded down to a multiple of eight
IA3_HD int np_sum_half(int n) {
  const int n2 = n / 2;
  return n2 - n2 % 8;
}

// the splits, at most NPSUM_SPLITS deep: the larger part of n elements has at most n/2 + 8, so 512 -> 264 -> 140 -> 78
constexpr int NPSUM_SPLITS = 3;
template <class T, int D, class F>
IA3_HD T np_sum_split(F at, int off, int n) {
  if constexpr (D == 0) {
    return np_sum_block<T>(at, off, n);
  } else {
    if (n <= NPSUM_BLOCK) return np_sum_block<T>(at, off, n);
    const int n2 = np_sum_half(n);
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

// sum of at(0) .. at(n - 1) for any n >= 0: the recursion `sum(n) = sum(first part) + sum(rest)` as a loop.  A frame is a
// part whose first half is being summed (state 1) or whose second half is (state 2, `left` holds the first);
// a part is at most n/2 + 8 elements of its parent, so 2^31 elements are at most 25 deep.
constexpr int NPSUM_DEPTH = 32;
template <class T, class F>
IA3_HD T np_sum_any(F at, int n) {
  int off[NPSUM_DEPTH], len[NPSUM_DEPTH], state[NPSUM_DEPTH];
  T left[NPSUM_DEPTH];
  int sp = 0;
  off[0] = 0; len[0] = n; state[0] = 0;
  T ret = (T)0;
  while (sp >= 0) {
    if (state[sp] == 0) {
      if (len[sp] <= NPSUM_BLOCK) { ret = np_sum_block<T>(at, off[sp], len[sp]); --sp; continue; }
      state[sp] = 1;
      off[sp + 1] = off[sp]; len[sp + 1] = np_sum_half(len[sp]); state[sp + 1] = 0;
      ++sp;
    } else if (state[sp] == 1) {
      left[sp] = ret;
      state[sp] = 2;
      const int n2 = np_sum_half(len[sp]);
      off[sp + 1] = off[sp] + n2; len[sp + 1] = len[sp] - n2; state[sp + 1] = 0;
      ++sp;
    } else {
      ret = left[sp] + ret;
      --sp;
    }
  }
  return ret;
}

template <class T>
IA3_HD T np_sum(const T* a, int n) {
  return np_sum_f<T>([a](int i) { return a[i]; }, n);
}

}  // namespace ia3
