// Host and device arithmetic of the domain distances (domain.hip), free of any HIP include so that a
// host-only program can check it (tests/native/domain_cpu.cpp).  domain_tools/distance.py of the reference, restated:
//   dm_edge, dm_slices          the edge rule and the truncated slices of _sliding_window_dist (:23-28)
//   dm_keep_intra / _inter      which entries enter the two sets of a window (:30-37)
//   dm_before, dm_mid_*         exact ranking: the place of a value in np.sort's order, the two middle ranks
//   dm_median2                  np.median of the two middle values
//   dm_mean, dm_var             np.mean / np.var in NumPy's pairwise order (ia3_npsum.h; the sets hold at most 256 values)
//   dm_ks_diff, dm_ks_stat      the two-sided statistic of scipy.stats.ks_2samp from `searchsorted(side='right')` counts
//   dm_window_final             the last line of each metric, quotients as written: inf and NaN come out as NumPy's
//   dm_window_serial            a whole window problem on one thread, out of the pieces above (the host check runs it;
//                               window_k runs the same pieces with a wavefront)
//   dm_key, dm_digit, ...       the ordered key of a float64 of either sign and the 8 x 8-bit digit steps of the select
//                               that dists_k runs by recomputation (the bin of a rank: ds_pick_bin of ia3_distsum.h);
//                               dm_nanmedian what np.nanmedian makes of the result
//   dm_dist_final               the last lines of domain_distance (:131-158), with Python's max(_final_dist, 0)
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "ia3_distsum.h"
#include "ia3_npsum.h"
#include "ia3_order.h"

#if defined(__HIPCC__)
#define IA3_DM_HD __host__ __device__ inline
#else
#define IA3_DM_HD inline
#endif

namespace ia3dm {

typedef unsigned long long u64;

constexpr int DM_MAX_WD = 16;                              // IA3_DOMAIN_MAX_WINDOW
constexpr int DM_MAX_W = 16;                               // window sizes of one call
constexpr int DM_MAX_INTRA = DM_MAX_WD * (DM_MAX_WD - 1);  // 2 C(16, 2) = 240
constexpr int DM_MAX_INTER = DM_MAX_WD * DM_MAX_WD;        // 256
static_assert(DM_MAX_INTER <= ia3::NPSUM_MAX, "np_sum_f covers every set of a window");

enum { DM_W_MEDIAN = 0, DM_W_MEAN = 1, DM_W_KS = 2, DM_W_NORMED_INSULATION = 3, DM_W_INSULATION = 4 };   // IA3_DOMAIN_WINDOW_*
enum { DM_D_MEDIAN = 0, DM_D_ABSOLUTE_MEDIAN = 1, DM_D_INSULATION = 2 };                                  // IA3_DOMAIN_DIST_*

IA3_DM_HD double dm_nan() {
  const u64 b = 0x7ff8000000000000ull;
  double v;
  memcpy(&v, &b, 8);
  return v;
}

// ---- windows ----------------------------------------------------------------------------------------------------------

// :23  `_i - int(_wd/2) < 0 or _i + int(_wd/2) >= len(_mat)`: the result is 0
IA3_DM_HD bool dm_edge(int i, int wd, int R) { return i - wd / 2 < 0 || i + wd / 2 >= R; }
// :27-28  the left slice [l0, i) and the right slice [i, r1)
IA3_DM_HD void dm_slices(int i, int wd, int R, int* l0, int* r1) {
  *l0 = i - wd > 0 ? i - wd : 0;
  *r1 = i + wd < R ? i + wd : R;
}
// :30-35  an entry above the diagonal of a diagonal block stays when it is not NaN and > 0 (np.triu's zeros go the same way)
IA3_DM_HD bool dm_keep_intra(double v) { return v > 0.0; }
// :36-37  an entry of the off-diagonal block stays when it is not NaN
IA3_DM_HD bool dm_keep_inter(double v) { return v == v; }

// value j stands before value k in np.sort's order of values that hold no NaN (equal values in the order of their index)
IA3_DM_HD bool dm_before(double vj, int j, double vk, int k) { return vj < vk || (vj == vk && j < k); }
IA3_DM_HD int dm_mid_lo(int n) { return (n - 1) / 2; }
IA3_DM_HD int dm_mid_hi(int n) { return n / 2; }
// np.median: the middle value, or np.mean of the two middle values
IA3_DM_HD double dm_median2(double lo, double hi, int n) { return (n & 1) ? lo : (lo + hi) / 2.0; }

// np.mean: add.reduce(x) / n
template <class F>
IA3_DM_HD double dm_mean(F at, int n) { return ia3::np_sum_f<double>(at, n) / (double)n; }
// np.var: add.reduce((x - mean) * (x - mean)) / n
template <class F>
IA3_DM_HD double dm_var(F at, int n, double mean) {
  return ia3::np_sum_f<double>([&](int i) { const double d = at(i) - mean; return d * d; }, n) / (double)n;
}

// ks_2samp: c1 and c2 of the n1 and n2 values are <= x; the difference of the two empirical distribution functions at x
IA3_DM_HD double dm_ks_diff(int c1, int n1, int c2, int n2) { return (double)c1 / (double)n1 - (double)c2 / (double)n2; }
// ... and the statistic from the smallest and the largest difference: d = max(clip(-min, 0, 1), max), which the exact
// method (taken for samples of up to 10000 values) puts back on the lattice of multiples of 1 / lcm(n1, n2):
// h = int(np.round(d * lcm)), d = h * 1.0 / lcm (scipy/stats/_stats_py.py, _attempt_exact_2kssamp)
IA3_DM_HD double dm_ks_stat(double mn, double mx, int n1, int n2) {
  double a = -mn;
  a = a < 0.0 ? 0.0 : a;
  a = a > 1.0 ? 1.0 : a;
  const double d = a > mx ? a : mx;
  int g = n1, r = n2;
  while (r) { const int t = g % r; g = r; r = t; }
  const double lcm = (double)((n1 / g) * n2);
  return rint(d * lcm) / lcm;
}
// np.sign of a float64: +0 for either zero, NaN stays
IA3_DM_HD double dm_sign(double x) { return x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : (x == 0.0 ? 0.0 : x)); }

// :43-61  a and b are, by metric: median: the two medians and the two medians of squared deviations; mean: means and
// variances; ks: the two medians, the statistic in v_inter; the insulations: the two means
IA3_DM_HD double dm_window_final(int metric, double m_inter, double m_intra, double v_inter, double v_intra) {
  switch (metric) {
    case DM_W_MEDIAN:
    case DM_W_MEAN: return (m_inter - m_intra) / sqrt(v_inter + v_intra);
    case DM_W_KS: return dm_sign(m_inter - m_intra) * v_inter;
    case DM_W_NORMED_INSULATION: return (m_intra - m_inter) / (m_intra + m_inter);
    default: return m_inter / m_intra;
  }
}

// np.median of v[0 .. n), n >= 1, by ranking; NaN when a value is NaN
IA3_DM_HD double dm_median_serial(const double* v, int n) {
  double lo = 0.0, hi = 0.0;
  for (int k = 0; k < n; ++k) {
    if (v[k] != v[k]) return dm_nan();
    int r = 0;
    for (int j = 0; j < n; ++j) r += dm_before(v[j], j, v[k], k) ? 1 : 0;
    if (r == dm_mid_lo(n)) lo = v[k];
    if (r == dm_mid_hi(n)) hi = v[k];
  }
  return dm_median2(lo, hi, n);
}

IA3_DM_HD double dm_ks_serial(const double* a, int na, const double* b, int nb) {
  double mn = INFINITY, mx = -INFINITY;
  for (int k = 0; k < na + nb; ++k) {
    const double x = k < na ? a[k] : b[k - na];
    int ca = 0, cb = 0;
    for (int j = 0; j < na; ++j) ca += a[j] <= x ? 1 : 0;
    for (int j = 0; j < nb; ++j) cb += b[j] <= x ? 1 : 0;
    const double d = dm_ks_diff(ca, na, cb, nb);
    mn = d < mn ? d : mn;
    mx = d > mx ? d : mx;
  }
  return dm_ks_stat(mn, mx, na, nb);
}

// One window problem.  at(r, c) is entry [r, c] of the distance map; intra and inter are work arrays of DM_MAX_INTRA and
// DM_MAX_INTER values (the squared deviations overwrite them).
template <class F>
IA3_DM_HD double dm_window_serial(F at, int R, int i, int wd, int metric, double* intra, double* inter) {
  if (dm_edge(i, wd, R)) return 0.0;
  int l0, r1;
  dm_slices(i, wd, R, &l0, &r1);
  int ni = 0, nj = 0;
  for (int r = l0; r < i; ++r)
    for (int c = r + 1; c < i; ++c) { const double v = at(r, c); if (dm_keep_intra(v)) intra[ni++] = v; }
  for (int r = i; r < r1; ++r)
    for (int c = r + 1; c < r1; ++c) { const double v = at(r, c); if (dm_keep_intra(v)) intra[ni++] = v; }
  for (int r = l0; r < i; ++r)
    for (int c = i; c < r1; ++c) { const double v = at(r, c); if (dm_keep_inter(v)) inter[nj++] = v; }
  if (ni == 0 || nj == 0) return 0.0;
  if (metric == DM_W_MEDIAN || metric == DM_W_KS) {
    const double m_inter = dm_median_serial(inter, nj), m_intra = dm_median_serial(intra, ni);
    if (metric == DM_W_KS) return dm_window_final(metric, m_inter, m_intra, dm_ks_serial(intra, ni, inter, nj), 0.0);
    for (int k = 0; k < nj; ++k) { const double d = inter[k] - m_inter; inter[k] = d * d; }
    for (int k = 0; k < ni; ++k) { const double d = intra[k] - m_intra; intra[k] = d * d; }
    return dm_window_final(metric, m_inter, m_intra, dm_median_serial(inter, nj), dm_median_serial(intra, ni));
  }
  const double m_inter = dm_mean([&](int k) { return inter[k]; }, nj), m_intra = dm_mean([&](int k) { return intra[k]; }, ni);
  double v_inter = 0.0, v_intra = 0.0;
  if (metric == DM_W_MEAN) {
    v_inter = dm_var([&](int k) { return inter[k]; }, nj, m_inter);
    v_intra = dm_var([&](int k) { return intra[k]; }, ni, m_intra);
  }
  return dm_window_final(metric, m_inter, m_intra, v_inter, v_intra);
}

// ---- domain distances ---------------------------------------------------------------------------------------------------

constexpr int DM_DIGIT = 8, DM_BINS = 1 << DM_DIGIT, DM_PASSES = 8;   // 64 key bits: the distances of a map may be negative

IA3_DM_HD u64 dm_key(double v) { return ia3ord::KeyOf<double>::key(v); }   // v is not NaN
IA3_DM_HD double dm_value(u64 key) { return ia3ord::KeyOf<double>::inv(key); }
IA3_DM_HD int dm_shift(int pass) { return 64 - DM_DIGIT * (pass + 1); }
// the key takes part in digit pass `pass` of a rank whose decided bits are `prefix`
IA3_DM_HD bool dm_matches(u64 key, u64 prefix, int pass) { return pass == 0 || (key >> (dm_shift(pass) + DM_DIGIT)) == (prefix >> (dm_shift(pass) + DM_DIGIT)); }
IA3_DM_HD int dm_digit(u64 key, int pass) { return (int)(key >> dm_shift(pass)) & (DM_BINS - 1); }
// np.nanmedian of c values that are not NaN from the lower middle value, the number of values <= it and the smallest
// value above it: the upper middle value is the lower one when more than c / 2 values are <= it
IA3_DM_HD double dm_nanmedian(unsigned c, u64 lo_key, unsigned count_le, u64 min_gt) {
  if (c == 0) return dm_nan();
  const double lo = dm_value(lo_key);
  if (c & 1) return lo;
  const double hi = dm_value(count_le > c / 2 ? lo_key : min_gt);
  return (lo + hi) / 2.0;
}
// the value whose median the second select takes: (d - m)**2
IA3_DM_HD double dm_dev2(double d, double m) { const double t = d - m; return t * t; }

// :128-158.  n_inter / n_intra: the values of the two sets that are not NaN.  *int_zero: Python's integer 0 is returned
// (an empty set, or max(_final_dist, 0) chose its second argument: `0 > _final_dist`, which a NaN never satisfies)
IA3_DM_HD double dm_dist_final(int metric, unsigned n_inter, unsigned n_intra, double m_inter, double m_intra, double v_inter,
                               double v_intra, int allow_minus, int* int_zero) {
  *int_zero = 1;
  if (n_inter == 0 || n_intra == 0) return 0.0;
  double f;
  if (metric == DM_D_MEDIAN) f = (m_inter - m_intra) / sqrt(v_inter + v_intra);
  else if (metric == DM_D_INSULATION) f = m_inter / m_intra;
  else f = m_inter - m_intra;
  if (!allow_minus && 0.0 > f) return 0.0;
  *int_zero = 0;
  return f;
}

// the block of `rows` x `cols` entries of which element t is entry (r, c); upper: only r < c counts (a pdist)
IA3_DM_HD void dm_rc(long long t, int cols, int* r, int* c) {
  *r = (int)(t / cols);
  *c = (int)(t % cols);
}

}  // namespace ia3dm
