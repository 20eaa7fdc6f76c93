// Host and device arithmetic of the population distance summaries (distsum.hip), free of any HIP include so
// that a host-only program can check it (tests/native/distsum_cpu.cpp):
//   ia3_dist_qstar   the contact threshold moved onto squared distances
//   ds_*             the keys of q = (dz*dz + dx*dx) + dy*dy (q >= +0 or NaN), the digit steps of the radix select that
//                    distsum.hip runs by recomputation, and the median NumPy makes of the two selected values
//   ds_pairwise      NumPy's pairwise summation of any length (the order np.nanmean takes for a stack of 1 x 1 matrices)
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define IA3_DS_HD __host__ __device__ inline
#else
#define IA3_DS_HD inline
#endif

// The largest double q* with sqrt(q*) <= th, so that for q >= 0 `sqrt(q) <= th` is `q <= q*` (sqrt is monotone and
// correctly rounded).  th < 0 or NaN: -1, no q >= 0 is a contact; th = +inf: +inf, every q that is not NaN is one.
// From th * th the answer is a step or two away; both loops end because sqrt is monotone.
inline double ia3_dist_qstar(double th) {
  if (!(th >= 0)) return -1.0;
  if (th == INFINITY) return INFINITY;
  volatile double c = th * th;
  while (sqrt(c) > th) c = nextafter(c, -INFINITY);   // sqrt(0) = 0 <= th: c never leaves [0, inf)
  for (;;) {
    const double up = nextafter(c, INFINITY);
    if (up == INFINITY || !(sqrt(up) <= th)) break;
    c = up;
  }
  return c;
}

namespace ia3ds {

typedef unsigned long long u64;

constexpr int DS_DIGIT = 7;                  // key bits per pass: bit 63 is known (q >= +0), 63 = 9 x 7
constexpr int DS_BINS = 1 << DS_DIGIT;
constexpr int DS_PASSES = 9;
constexpr u64 DS_TOP = 1ull << 63;

// KeyOf<double>::key (ia3_order.h) of a q that is >= +0 and not NaN: the bit pattern with the sign bit set
IA3_DS_HD u64 ds_key(double q) {
  u64 b;
  memcpy(&b, &q, 8);
  return b | DS_TOP;
}
IA3_DS_HD double ds_value(u64 key) {
  key &= ~DS_TOP;
  double v;
  memcpy(&v, &key, 8);
  return v;
}
IA3_DS_HD int ds_shift(int pass) { return 56 - DS_DIGIT * pass; }
// the key takes part in digit pass `pass` of a rank whose decided bits are `prefix`
IA3_DS_HD bool ds_matches(u64 key, u64 prefix, int pass) {
  const int s = ds_shift(pass) + DS_DIGIT;
  return (key >> s) == (prefix >> s);
}
IA3_DS_HD int ds_digit(u64 key, int pass) { return (int)(key >> ds_shift(pass)) & (DS_BINS - 1); }

// hist[first .. first + n): the bin that holds rank k among them (k < their sum); k becomes the rank inside that bin
IA3_DS_HD int ds_pick_bin(const unsigned* hist, int first, int n, unsigned& k) {
  int b = first;
  for (; b < first + n - 1; ++b) {
    const unsigned c = hist[b];
    if (c > k) break;
    k -= c;
  }
  return b;
}

// ranks of the two middle values of c >= 1 sorted values: (c - 1) / 2 and c / 2.  The select finds the lower one; the
// upper one is the same value when more than c / 2 values are <= it, otherwise the smallest value above it.
IA3_DS_HD u64 ds_upper_key(u64 lo_key, unsigned c, unsigned count_le, u64 min_gt) {
  return count_le > c / 2 ? lo_key : min_gt;
}
// np.nanmedian of the roots: the middle value, or (lo + hi) / 2.0 of the two middle values; NaN of no value
IA3_DS_HD double ds_median(unsigned c, u64 lo_key, u64 hi_key) {
  if (c == 0) {
    const u64 nan = 0x7ff8000000000000ull;
    double v;
    memcpy(&v, &nan, 8);
    return v;
  }
  const double lo = sqrt(ds_value(lo_key));
  if (c & 1) return lo;
  const double hi = sqrt(ds_value(hi_key));
  return (lo + hi) / 2.0;
}

// np.add.reduce of at(0) .. at(n - 1) over a contiguous axis (numpy/_core/src/umath/loops_utils.h.src; ia3_npsum.h states
// the same rule for n <= 512): fewer than 8 values left to right, up to 128 values through eight accumulators, more
// values split at n / 2 rounded down to a multiple of 8.  The recursion is unrolled onto a stack (2^31 values: 24 levels).
template <class F>
IA3_DS_HD double ds_pairwise_block(F at, long long off, int n) {
  if (n < 8) {
    double res = 0.0;
    for (int i = 0; i < n; ++i) res = res + at(off + i);
    return res;
  }
  double r[8];
  for (int j = 0; j < 8; ++j) r[j] = at(off + j);
  int i = 8;
  for (; i < n - (n % 8); i += 8)
    for (int j = 0; j < 8; ++j) r[j] = r[j] + at(off + i + j);
  double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; ++i) res = res + at(off + i);
  return res;
}

template <class F>
IA3_DS_HD double ds_pairwise(F at, long long n) {
  struct Frame { long long off, n; int state; double left; };
  Frame stk[40];
  int sp = 0;
  double ret = 0.0;
  stk[0] = Frame{0, n, 0, 0.0};
  while (sp >= 0) {
    Frame& f = stk[sp];
    if (f.n <= 128) { ret = ds_pairwise_block(at, f.off, (int)f.n); --sp; continue; }
    long long n2 = f.n / 2;
    n2 -= n2 % 8;
    if (f.state == 0) { f.state = 1; stk[sp + 1] = Frame{f.off, n2, 0, 0.0}; ++sp; }
    else if (f.state == 1) { f.left = ret; f.state = 2; stk[sp + 1] = Frame{f.off + n2, f.n - n2, 0, 0.0}; ++sp; }
    else { ret = f.left + ret; --sp; }
  }
  return ret;
}

}  // namespace ia3ds
