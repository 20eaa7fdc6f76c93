// Host and device arithmetic of the chromosomal spot scores (score.hip), free of any HIP include so that a
// host-only program can check it (tests/native/score_cpu.cpp).  spot_tools/scoring.py of the reference, restated:
//   sc_norm_rows               np.linalg.norm(x, axis=1) of three columns: sqrt((a*a + b*b) + c*c)
//   sc_norm_vec                np.linalg.norm(v) of one 3-vector: sqrt(v.dot(v)); the dot of three float64 values is
//                              BLAS's, which on the x86-64 OpenBLAS of NumPy's wheels runs as fma(c, c, fma(b, b, a*a))
//   Mean3                      np.nanmean(x, axis=0) of (m, 3): one accumulator and one count per column, row after row
//   sc_local                   _local_distance (:124-155) of one spot
//   sc_nb_median, sc_neighbors neighboring_distances / _neighboring_distance (:157-205) of one spot: np.nanmedian by exact
//                              ranking (dm_before / dm_median2 of ia3_domain.h)
//   sc_nanmean2                np.nanmean([fwd, rev], axis=0) of one spot (:503)
//   sc_upper, sc_cum_prob      _cum_prob (:81-107) from `<=` counts in the sorted reference array
//   sc_score                   distance_score (:6-51) and intensity_score (:53-78) up to the argument of np.log
//   sc_nanmean_1d, sc_rg       np.nanmean of a contiguous 1-D array (NumPy's pairwise order, ia3_npsum.h) and
//                              radius_of_gyration (:411-420)
// Rows come through accessors so that the kernels (one lane per spot) and the host check run the same text:
//   Index::range(id, &b, &e)   the places [b, e) of the rows with region id `id`, in row order
//   Index::zxy(k, out)         the coordinates in nm of the row at place k
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "ia3_domain.h"
#include "ia3_npsum.h"

#if defined(__HIPCC__)
#define IA3_SC_HD __host__ __device__ inline
#else
#define IA3_SC_HD inline
#endif

namespace ia3sc {

constexpr int SC_MAX_PER_REGION = 64;   // IA3_SCORE_MAX_PER_REGION
constexpr int SC_MAX_LOCAL = 33;        // IA3_SCORE_MAX_LOCAL
constexpr int SC_MAX_HALF = (SC_MAX_LOCAL - 1) / 2;

enum { SC_DIST_LINEAR = 0, SC_DIST_CDF = 1, SC_INT_LINEAR = 2, SC_INT_CDF = 3, SC_CUM_PROB = 4 };   // IA3_SCORE_KIND_*
enum { SC_REF_MEDIAN = 0, SC_REF_MEAN = 1, SC_REF_RG = 2, SC_REF_CDF = 3 };                         // IA3_SCORE_REF_*
// what the host makes of a value: the value itself, np.log(value) * w, or -inf; SC_NAN_IN: the input was NaN
enum { SC_VALUE = 0, SC_LOG = 1, SC_NEG_INF = 2, SC_NAN_IN = 4 };

IA3_SC_HD double sc_nan() { return ia3dm::dm_nan(); }
IA3_SC_HD double sc_inf() { return INFINITY; }

IA3_SC_HD double sc_norm_rows(double a, double b, double c) { return sqrt((a * a + b * b) + c * c); }
IA3_SC_HD double sc_norm_vec(double a, double b, double c) { return sqrt(fma(c, c, fma(b, b, a * a))); }

// spots[:, 1:4] * distance_zxy
IA3_SC_HD void sc_zxy(const double* row4, const double* dzxy, double* out) {
  out[0] = row4[1] * dzxy[0];
  out[1] = row4[2] * dzxy[1];
  out[2] = row4[3] * dzxy[2];
}

struct Mean3 {
  double s[3];
  int c[3], rows;
  IA3_SC_HD Mean3() : rows(0) { for (int k = 0; k < 3; ++k) { s[k] = 0.0; c[k] = 0; } }
  IA3_SC_HD void add(const double* v) {
    for (int k = 0; k < 3; ++k) {
      const bool nan = v[k] != v[k];
      const double x = nan ? 0.0 : v[k];
      s[k] = rows ? s[k] + x : x;
      c[k] += nan ? 0 : 1;
    }
    ++rows;
  }
  IA3_SC_HD void finish(double* m) const { for (int k = 0; k < 3; ++k) m[k] = s[k] / (double)c[k]; }
};

// _local_distance of the spot at t with region id `id` against the selected rows: half = int((local_size - 1) / 2)
template <class Index>
IA3_SC_HD double sc_local(const double* t, long long id, int half, double invalid, const Index& sel) {
  Mean3 mean;
  int n_nan = 0;
  for (long long j = id - half; j <= id + half; ++j) {
    if (j == id) continue;
    int b, e;
    sel.range(j, &b, &e);
    for (int k = b; k < e; ++k) {
      double v[3];
      sel.zxy(k, v);
      n_nan += (v[0] != v[0] || v[1] != v[1] || v[2] != v[2]) ? 1 : 0;
      mean.add(v);
    }
  }
  if (mean.rows == 0 || n_nan == mean.rows) return invalid;
  double m[3];
  mean.finish(m);
  return sc_norm_vec(m[0] - t[0], m[1] - t[1], m[2] - t[2]);
}

// the squared argument of sc_norm_rows between place k and t; sqrt is monotone, so the order of these is the order of the
// norms and the value at a rank is the square root of the value at that rank
template <class Index>
IA3_SC_HD double sc_q(const Index& spots, int k, const double* t) {
  double v[3];
  spots.zxy(k, v);
  const double a = v[0] - t[0], b = v[1] - t[1], c = v[2] - t[2];
  return (a * a + b * b) + c * c;
}

// np.nanmedian of the norms between t and the rows at places [b, e): NaN for none, or when all are NaN
template <class Index>
IA3_SC_HD double sc_nb_median(const double* t, int b, int e, const Index& spots) {
  int c = 0;
  for (int k = b; k < e; ++k) { const double q = sc_q(spots, k, t); c += q == q ? 1 : 0; }
  if (c == 0) return sc_nan();
  const int lo = ia3dm::dm_mid_lo(c), hi = ia3dm::dm_mid_hi(c);
  double vlo = 0.0, vhi = 0.0;
  for (int k = b; k < e; ++k) {
    const double qk = sc_q(spots, k, t);
    if (qk != qk) continue;
    int r = 0;
    for (int j = b; j < e; ++j) r += ia3dm::dm_before(sc_q(spots, j, t), j, qk, k) ? 1 : 0;   // a NaN stands before nothing
    if (r == lo) vlo = qk;
    if (r == hi) vhi = qk;
  }
  return ia3dm::dm_median2(sqrt(vlo), sqrt(vhi), c);
}

// neighboring_distances of one spot among the spots themselves: both sides only when id + step is a region of theirs
template <class Index>
IA3_SC_HD void sc_neighbors(const double* t, long long id, long long step, double invalid, const Index& spots, double* fwd, double* rev) {
  int b, e;
  spots.range(id + step, &b, &e);
  if (e <= b) { *fwd = invalid; *rev = invalid; return; }
  *fwd = sc_nb_median(t, b, e, spots);
  spots.range(id - step, &b, &e);
  *rev = sc_nb_median(t, b, e, spots);
}

IA3_SC_HD double sc_nanmean2(double f, double r) {
  const bool fn = f != f, rn = r != r;
  return ((fn ? 0.0 : f) + (rn ? 0.0 : r)) / (double)((fn ? 0 : 1) + (rn ? 0 : 1));
}

// the number of sorted[0 .. n) that are <= v (none for a NaN)
IA3_SC_HD int sc_upper(const double* sorted, int n, double v) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (sorted[mid] <= v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// :93-105 from the counts of the n values that are <= the target, <= vmin and <= vmax
IA3_SC_HD double sc_cum_prob(int c, int c_min, int c_max, int n) {
  const double p = (double)c / (double)n, min_p = (double)c_min / (double)n, max_p = (double)c_max / (double)n;
  double r = max_p <= min_p ? p - min_p : (p - min_p) / (max_p - min_p);
  if (r <= 0.0) r = 0.0;
  if (r != r) r = 1.0 / (double)n;
  if (r >= 1.0) r = 1.0;
  return r;
}

IA3_SC_HD double sc_cum_prob_of(const double* sorted, int n, double x, double vmin, double vmax) {
  const double v = x != x ? sc_inf() : x;
  return sc_cum_prob(sc_upper(sorted, n, v), sc_upper(sorted, n, vmin), sc_upper(sorted, n, vmax), n);
}

// One score of one spot.  ref: the reference number of the linear metric; sorted[0 .. n): the reference array of the cdf
// metric without its NaNs, ascending; lo / hi: min / max of distance_limits, or intensity_th / inf.  Returns the value and
// in *cls what is left to the host (np.log is the host's).
IA3_SC_HD double sc_score(int kind, double x, double ref, const double* sorted, int n, double w, double lo, double hi, int* cls) {
  const int nan_in = x != x ? SC_NAN_IN : 0;
  *cls = SC_VALUE | nan_in;
  switch (kind) {
    case SC_DIST_LINEAR: {
      double s = (-w) * (x / ref);
      if (x > hi) s = s - (w * (x - hi)) / ref;
      return s;
    }
    case SC_INT_LINEAR:
      if (x <= 0.0) { *cls = SC_NEG_INF | nan_in; return 0.0; }
      if (x > 0.0) { *cls = SC_LOG | nan_in; return x / (x + ref); }
      return 0.0;
    default: break;
  }
  if (n <= 0) return sc_nan();
  const double p = sc_cum_prob_of(sorted, n, x, lo, hi);
  if (kind == SC_CUM_PROB) return p;
  const double cdf = kind == SC_DIST_CDF ? 1.0 - p : p;
  *cls = (cdf > 0.0 ? SC_LOG : SC_NEG_INF) | nan_in;
  return cdf;
}

// np.nanmean of at(0 .. n): NaNs count as 0 in the pairwise sum and not in the divisor
template <class F>
IA3_SC_HD double sc_nanmean_1d(F at, int n) {
  int c = 0;
  for (int i = 0; i < n; ++i) { const double v = at(i); c += v == v ? 1 : 0; }
  const double s = ia3::np_sum_any<double>([&](int i) { const double v = at(i); return v == v ? v : 0.0; }, n);
  return s / (double)c;
}

// radius_of_gyration of the rows at places [0, n) of `spots` (any order of places: at(i) names the row), mean: their nanmean
template <class F>
IA3_SC_HD double sc_rg(F row_zxy, int n, const double* mean) {
  return sqrt(sc_nanmean_1d([&](int i) {
    double v[3];
    row_zxy(i, v);
    const double r = sc_norm_rows(v[0] - mean[0], v[1] - mean[1], v[2] - mean[2]);
    return r * r;
  }, n));
}

// np.nanmedian of sorted[0 .. n) that holds no NaN
IA3_SC_HD double sc_median_sorted(const double* sorted, int n) {
  if (n <= 0) return sc_nan();
  return ia3dm::dm_median2(sorted[ia3dm::dm_mid_lo(n)], sorted[ia3dm::dm_mid_hi(n)], n);
}

// the chromosome of row i: start[c] <= i < start[c + 1]
IA3_SC_HD int sc_chrom_of(const int* start, int C, int i) {
  int lo = 0, hi = C;
  while (hi - lo > 1) {
    const int mid = lo + (hi - lo) / 2;
    if (start[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

// the places [b, e) of region id `id` in the ids sid[lo .. hi) of one chromosome, ascending
IA3_SC_HD void sc_range(const int* sid, int lo, int hi, long long id, int* b, int* e) {
  int l = lo, h = hi;
  while (l < h) { const int m = l + (h - l) / 2; if ((long long)sid[m] < id) l = m + 1; else h = m; }
  *b = l;
  h = hi;
  while (l < h) { const int m = l + (h - l) / 2; if ((long long)sid[m] <= id) l = m + 1; else h = m; }
  *e = l;
}

// the rows of one chromosome by region id: sid / perm are the ids and the rows (of the whole table) in the order of
// (id, row) inside [lo, hi)
struct RowIndex {
  const double* rows;   // (n, 4): h, z, x, y in pixels
  const int* sid;
  const int* perm;
  const double* dzxy;
  int lo, hi;
  IA3_SC_HD void range(long long id, int* b, int* e) const { sc_range(sid, lo, hi, id, b, e); }
  IA3_SC_HD void zxy(int k, double* out) const { sc_zxy(rows + 4 * (size_t)perm[k], dzxy, out); }
};

}  // namespace ia3sc
