// Host and device arithmetic of the radix select (ia3_select.h), free of any HIP include so that a
// host-only program can check it (tests/native/select_cpu.cpp):
//   KeyOf<T>           order-preserving integer keys of uint16, float32 and float64 values
//   pick_bin, regroup  the two steps between the histogram passes
//   middle ranks, median_of, percentile_*   what NumPy and SciPy make of the selected values
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define IA3_ORD_HD __host__ __device__ inline
#else
#define IA3_ORD_HD inline
#endif

namespace ia3ord {

typedef unsigned long long u64;

// a < b  <=>  key(a) < key(b), -0 before +0; NaNs of either sign get the largest key, as np.sort puts them last
template <class T> struct KeyOf;
template <> struct KeyOf<uint16_t> {
  typedef uint32_t K;
  static constexpr int BITS = 16;
  static IA3_ORD_HD K key(uint16_t v) { return v; }
  static IA3_ORD_HD uint16_t inv(K k) { return (uint16_t)k; }
};
template <> struct KeyOf<float> {
  typedef uint32_t K;
  static constexpr int BITS = 32;
  static IA3_ORD_HD K key(float v) {
    if (v != v) return 0xFFFFFFFFu;
    uint32_t b;
    memcpy(&b, &v, 4);
    return b & 0x80000000u ? ~b : (b | 0x80000000u);
  }
  static IA3_ORD_HD float inv(K k) {
    k = k & 0x80000000u ? (k & 0x7FFFFFFFu) : ~k;
    float v;
    memcpy(&v, &k, 4);
    return v;
  }
};
template <> struct KeyOf<double> {
  typedef u64 K;
  static constexpr int BITS = 64;
  static IA3_ORD_HD K key(double v) {
    if (v != v) return ~0ull;
    u64 b;
    memcpy(&b, &v, 8);
    return b >> 63 ? ~b : (b | (1ull << 63));
  }
  static IA3_ORD_HD double inv(K k) {
    k = k >> 63 ? (k & ~(1ull << 63)) : ~k;
    double v;
    memcpy(&v, &k, 8);
    return v;
  }
};

// the bin of a histogram of nb bins that holds rank k; k becomes the rank among the values of that bin
IA3_ORD_HD int pick_bin(const unsigned* h, int nb, u64& k) {
  u64 cum = 0;
  int b = 0;
  for (; b < nb; ++b) {
    const u64 c = h[b];
    if (cum + c > k) break;
    cum += c;
  }
  k -= cum;
  return b < nb ? b : nb - 1;
}

// lists the distinct values among prefix[0 .. n) in gprefix, in the order they appear; grp[i] is where prefix[i] stands
// in that list.  Returns its length: a histogram pass counts once per distinct prefix.
IA3_ORD_HD int regroup(const u64* prefix, int n, u64* gprefix, int* grp) {
  int ng = 0;
  for (int i = 0; i < n; ++i) {
    int g = 0;
    while (g < ng && gprefix[g] != prefix[i]) ++g;
    if (g == ng) gprefix[ng++] = prefix[i];
    grp[i] = g;
  }
  return ng;
}

// np.median of n values: the order statistic of rank mid_lo(n) for an odd n, else the mean of those of ranks mid_lo(n)
// and mid_hi(n), added and halved in A.  A = float: what np.mean makes of two float32 values; A = double: of two uint16
// or float64 values.
IA3_ORD_HD u64 mid_lo(u64 n) { return (n - 1) / 2; }
IA3_ORD_HD u64 mid_hi(u64 n) { return n / 2; }
template <class A> IA3_ORD_HD A median_of(A lo, A hi, bool odd) { return odd ? lo : (lo + hi) / (A)2; }

// scipy.stats.scoreatpercentile of n values: rank i, and the weights of ranks i and percentile_next(i, n)
IA3_ORD_HD void percentile_index(double per, long long n, long long* i, double* idx) {
  *idx = per / 100. * (double)(n - 1);
  *i = (long long)*idx;
}
IA3_ORD_HD long long percentile_next(long long i, long long n) { return i + 1 < n ? i + 1 : i; }
IA3_ORD_HD double percentile_value(double idx, long long i, double s0, double s1) {
  if ((double)i == idx) return s0;
  const double w0 = (double)(i + 1) - idx, w1 = idx - (double)i;
  return (s0 * w0 + s1 * w1) / (w0 + w1);
}

}  // namespace ia3ord
