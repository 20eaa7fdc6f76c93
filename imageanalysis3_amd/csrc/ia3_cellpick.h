// Host and device arithmetic of the per-cell spot pickers (cellpick.hip), free of any HIP include so that a
// host-only program can check it (tests/native/cellpick_cpu.cpp).  spot_tools/picking.py of the reference, restated:
//   cp_before        the order of np.argsort with its ties pinned: ascending, NaN last, equal keys by ascending index
//   cp_argmin_first  np.argmin of a short vector: the first minimum, a NaN before any number
//   cp_merge_region  merge_spot_list (:662-765) of one region: the intensity flag, the greedy pass in list order with
//                    np.linalg.norm(axis=1) in pixels and `< dist_th`, the owner of every kept spot, the placeholder rows
//   cp_naive_region  the two selections of naive_pick_spots_for_chromosomes (:854-888) of one region
//   cp_nb_score      scoring.distance_score (:6-51) of one neighbour distance: pure IEEE arithmetic for 'linear'; for 'cdf'
//                    the value is one of n + 1 quotients and its score is read from a table that the host's np.log made
//   cp_allowed       the indices a chromosome may take in a step: argsort(scores)[-C:], or all when every score is infinite
//                    (_optimized_score_combinations :1531-1550); all of them when the region has no more spots than
//                    chromosomes (_all_score_combinations :1552-1563)
//   cp_pick          the choice of one spot of the next region (:1129-1155): itertools.product over the allowed indices
//                    with the last chromosome fastest, tuples with a repeated index left out unless spots are shared,
//                    np.nansum over the chromosomes from left to right, the maximum by ==, several maxima resolved by the
//                    first maximum of _global_maxs; the argsorts that rule reads are made only then
// Rows come through accessors so that the kernels and the host check run the same text.
#pragma once
#include <math.h>
#include <stdint.h>

#include "ia3_score.h"

namespace ia3cp {

constexpr int CP_MAX_CHROM = 6;    // IA3_CELLPICK_MAX_CHROM
constexpr int CP_MAX_SPOTS = 64;   // IA3_CELLPICK_MAX_SPOTS

enum { CP_NAIVE_OWN = 0, CP_NAIVE_MERGED = 1 };   // IA3_CELLPICK_NAIVE_*
enum { CP_OK = 0, CP_NO_TUPLE = 1, CP_NO_MAXIMUM = 2, CP_TOO_MANY = 3 };
// the most tuples one spot of the next region may walk: C^C is at most 46656; more arise only when every score of a chromosome
// is infinite and all its K indices are allowed (up to 64^6), which is refused instead of run
constexpr long long CP_MAX_TUPLES = 1LL << 22;   // IA3_CELLPICK_MAX_TUPLES

IA3_SC_HD bool cp_before(double a, int ia, double b, int ib) {
  const bool an = a != a, bn = b != b;
  if (an || bn) return an == bn ? ia < ib : bn;
  if (a < b) return true;
  if (a > b) return false;
  return ia < ib;
}

// the place of element i in the pinned argsort of at(0 .. n)
template <class F>
IA3_SC_HD int cp_rank(F at, int n, int i) {
  const double v = at(i);
  int r = 0;
  for (int j = 0; j < n; ++j) r += (j != i && cp_before(at(j), j, v, i)) ? 1 : 0;
  return r;
}

template <class F>
IA3_SC_HD int cp_argmin_first(F at, int n) {
  int best = 0;
  double vb = at(0);
  for (int k = 1; k < n; ++k) {
    const double v = at(k);
    if (vb == vb && (v < vb || v != v)) { best = k; vb = v; }
  }
  return best;
}

// ---- merge_spot_list ---------------------------------------------------------------------------------------------------------

// One region's list: the rows of chromosome c are rows[start[c] .. start[c + 1]) (h, z, x, y in pixels); with coordinates
// ((C, 3) pixels) a chromosome without rows stands in the list as one placeholder row (0, its coordinate).
struct MergeList {
  const double* rows;
  const int* start;
  const double* coords;   // null: chrom_coords is None (append_nan_spots False)
  int C;
  int pos[CP_MAX_CHROM + 1];
  IA3_SC_HD void init() {
    pos[0] = 0;
    for (int c = 0; c < C; ++c) {
      const int n = start[c + 1] - start[c];
      pos[c + 1] = pos[c] + (n > 0 ? n : (coords ? 1 : 0));
    }
  }
  IA3_SC_HD int size() const { return pos[C]; }
  // the entry at place e: its row, and the candidate it is (>= 0) or -(1 + chromosome) for a placeholder
  IA3_SC_HD int get(int e, double* hzxy) const {
    int c = 0;
    while (c + 1 < C && e >= pos[c + 1]) ++c;
    if (start[c + 1] - start[c] > 0) {
      const int i = start[c] + (e - pos[c]);
      for (int k = 0; k < 4; ++k) hzxy[k] = rows[4 * (size_t)i + k];
      return i;
    }
    hzxy[0] = 0.0;
    for (int k = 0; k < 3; ++k) hzxy[1 + k] = coords[3 * c + k];
    return -(1 + c);
  }
};

// keep: n bytes of scratch.  src / out: room for size() + C entries / rows of four.  row_nan[i]: candidate i holds a NaN in
// any of its columns.  Returns the number of merged rows and in *n_valid those of them without a NaN.
IA3_SC_HD int cp_merge_region(MergeList& L, const unsigned char* row_nan, int has_th, double th, int hard, double dist_th, unsigned char* keep,
                              int* src, double* out, int* n_valid) {
  L.init();
  const int n = L.size(), C = L.C;
  double a[4], b[4];
  for (int i = 0; i < n; ++i) keep[i] = 1;
  if (has_th && hard) {
    for (int i = 0; i < n; ++i) { L.get(i, a); keep[i] = a[0] >= th ? 1 : 0; }
  } else if (has_th) {
    int pass = 0;
    for (int i = 0; i < n; ++i) { L.get(i, a); pass += a[0] >= th ? 1 : 0; }
    const int m = pass > C ? pass : C;      // np.argsort(_ints)[-max(len(spot_list), sum(_ints >= th)):]
    if (m > 0 && m < n) {
      auto h = [&](int i) { double r[4]; L.get(i, r); return r[0]; };
      for (int i = 0; i < n; ++i) keep[i] = cp_rank(h, n, i) >= n - m ? 1 : 0;
    }
  }
  unsigned owned = 0;
  for (int i = 0; i < n; ++i) {
    if (!keep[i]) continue;
    L.get(i, a);
    for (int j = 0; j < n; ++j) {
      if (j == i) continue;
      L.get(j, b);
      if (ia3sc::sc_norm_rows(b[1] - a[1], b[2] - a[2], b[3] - a[3]) < dist_th) keep[j] = 0;
    }
    if (L.coords) {
      const double* cc = L.coords;
      owned |= 1u << cp_argmin_first([&](int c) { return ia3sc::sc_norm_rows(cc[3 * c] - a[1], cc[3 * c + 1] - a[2], cc[3 * c + 2] - a[3]); }, C);
    }
  }
  int K = 0, valid = 0;
  for (int i = 0; i < n; ++i) {
    if (!keep[i]) continue;
    src[K] = L.get(i, out + 4 * (size_t)K);
    valid += (src[K] >= 0 && !row_nan[src[K]]) ? 1 : 0;
    ++K;
  }
  if (L.coords)
    for (int c = 0; c < C; ++c) {
      if (owned & (1u << c)) continue;
      src[K] = -(1 + c);
      out[4 * (size_t)K] = 0.0;
      for (int k = 0; k < 3; ++k) out[4 * (size_t)K + 1 + k] = L.coords[3 * c + k];
      ++K;
    }
  *n_valid = valid;
  return K;
}

// ---- naive_pick_spots_for_chromosomes ------------------------------------------------------------------------------------------

// CP_NAIVE_OWN (:856, naive_pick_spots :38-44): per chromosome the last place of the pinned argsort of its own rows' h;
// pick[c] is that candidate, -1 for none.  CP_NAIVE_MERGED (:864-888): every merged row goes to its nearest coordinate in nm,
// per chromosome np.argmax of h among its rows; pick[c] is the merged row, sub[c] its index among the chromosome's rows.
IA3_SC_HD void cp_naive_region(int mode, const double* rows, const int* start, const double* merged, int K, const double* coords, const double* dzxy,
                               int C, int* pick, int* sub) {
  for (int c = 0; c < C; ++c) { pick[c] = -1; sub[c] = -1; }
  if (mode == CP_NAIVE_OWN) {
    for (int c = 0; c < C; ++c) {
      const int n = start[c + 1] - start[c];
      const double* r = rows + 4 * (size_t)start[c];
      for (int i = 0; i < n; ++i)
        if (cp_rank([&](int k) { return r[4 * (size_t)k]; }, n, i) == n - 1) pick[c] = start[c] + i;
    }
    return;
  }
  int count[CP_MAX_CHROM];
  double best[CP_MAX_CHROM];
  for (int c = 0; c < C; ++c) { count[c] = 0; best[c] = 0.0; }
  for (int i = 0; i < K; ++i) {
    const double* m = merged + 4 * (size_t)i;
    const double z = m[1] * dzxy[0], x = m[2] * dzxy[1], y = m[3] * dzxy[2];
    const int c = cp_argmin_first([&](int k) {
      return ia3sc::sc_norm_rows(coords[3 * k] * dzxy[0] - z, coords[3 * k + 1] * dzxy[1] - x, coords[3 * k + 2] * dzxy[2] - y); }, C);
    const double h = m[0];
    // np.argmax: the first maximum, the first NaN above every number
    if (count[c] == 0 || (best[c] == best[c] && (h > best[c] || h != h))) { pick[c] = i; sub[c] = count[c]; best[c] = h; }
    ++count[c];
  }
}

// ---- the forward pass ----------------------------------------------------------------------------------------------------------

// the neighbour reference of one chromosome
struct NbRef {
  int kind;               // SC_DIST_LINEAR or SC_DIST_CDF
  double ref;             // linear: the reference distance
  const double* sorted;   // cdf: the reference array without NaNs, ascending (n values)
  const double* table;    // cdf: n + 1 scores, table[k] for a distance with k reference values <= it
  int n;
  double w, hi, nan_mask;
};

IA3_SC_HD double cp_nb_score(const NbRef& r, double x) {
  if (r.w == 0.0) return 0.0;
  double s;
  if (r.kind == ia3sc::SC_DIST_LINEAR) {
    int cls;
    s = ia3sc::sc_score(ia3sc::SC_DIST_LINEAR, x, r.ref, nullptr, 0, r.w, 0.0, r.hi, &cls);
  } else {
    s = r.table[ia3sc::sc_upper(r.sorted, r.n, x != x ? ia3sc::sc_inf() : x)];
  }
  return x != x ? r.nan_mask : s;
}

// distance_score / gap + the previous dynamic score (:1100-1113); no division for a gap of 0
IA3_SC_HD double cp_measure(const NbRef& r, double dist, long long gap, double dy_prev) {
  const double s = cp_nb_score(r, dist);
  return (gap != 0 ? s / (double)gap : s) + dy_prev;
}

// allowed[0 .. return): the indices chromosome with scores at(0 .. K) may take when C chromosomes are picked together
template <class F>
IA3_SC_HD int cp_allowed(F at, int K, int C, int* allowed) {
  bool all_inf = true;
  for (int p = 0; p < K; ++p) { const double v = at(p); all_inf = all_inf && (v == ia3sc::sc_inf() || v == -ia3sc::sc_inf()); }
  if (K <= C || all_inf) {
    for (int p = 0; p < K; ++p) allowed[p] = p;
    return K;
  }
  for (int p = 0; p < K; ++p) {
    const int r = cp_rank(at, K, p);
    if (r >= K - C) allowed[r - (K - C)] = p;
  }
  return C;
}

// One spot of the next region.  na[c] / idx(c, a): the allowed indices of chromosome c; meas(c, p): the measure of
// chromosome c at spot p of the previous region (any p < K_prev).  sel[c]: the chosen previous spot.
template <class Idx, class Meas>
IA3_SC_HD int cp_pick(int C, int K_prev, const int* na, Idx idx, Meas meas, bool share, int* sel) {
  for (int c = 0; c < C; ++c) if (na[c] < 1) return CP_NO_TUPLE;
  long long product = 1;
  for (int c = 0; c < C; ++c) { product *= na[c]; if (product > CP_MAX_TUPLES) return CP_TOO_MANY; }
  double mc[CP_MAX_CHROM][CP_MAX_CHROM];
  bool cached = true;
  for (int c = 0; c < C; ++c) cached = cached && na[c] <= CP_MAX_CHROM;
  if (cached)
    for (int c = 0; c < C; ++c)
      for (int a = 0; a < na[c]; ++a) mc[c][a] = meas(c, idx(c, a));
  int t[CP_MAX_CHROM], p[CP_MAX_CHROM], first[CP_MAX_CHROM];
  double best = 0.0;
  long long n_best = 0, n_tuples = 0;
  // every tuple in itertools.product's order; pass 0 finds the maximum, pass 1 (several maxima) the first maximum of
  // max over c of argsort(measure_c[:, n])[p_c]
  unsigned char perm[CP_MAX_CHROM][CP_MAX_SPOTS];
  int g_best = -1;
  for (int pass = 0; pass < 2; ++pass) {
    if (pass == 1) {
      if (n_best <= 1) break;
      for (int c = 0; c < C; ++c)
        for (int q = 0; q < K_prev; ++q) perm[c][cp_rank([&](int k) { return meas(c, k); }, K_prev, q)] = (unsigned char)q;
    }
    for (int c = 0; c < C; ++c) t[c] = 0;
    for (;;) {
      bool ok = true;
      for (int c = 0; c < C; ++c) p[c] = idx(c, t[c]);
      if (!share)
        for (int c = 1; c < C && ok; ++c)
          for (int d = 0; d < c; ++d) if (p[d] == p[c]) { ok = false; break; }
      if (ok) {
        double s = 0.0;
        for (int c = 0; c < C; ++c) {
          double v = cached ? mc[c][t[c]] : meas(c, p[c]);
          v = v != v ? 0.0 : v;
          s = c ? s + v : v;
        }
        if (pass == 0) {
          ++n_tuples;
          if (s == s) {
            if (n_best == 0 || s > best) { best = s; n_best = 1; for (int c = 0; c < C; ++c) first[c] = p[c]; }
            else if (s == best) ++n_best;
          }
        } else if (s == best) {
          int g = 0;
          for (int c = 0; c < C; ++c) { const int o = perm[c][p[c]]; g = o > g ? o : g; }
          if (g > g_best) { g_best = g; for (int c = 0; c < C; ++c) first[c] = p[c]; }
        }
      }
      int c = C - 1;
      while (c >= 0 && ++t[c] == na[c]) { t[c] = 0; --c; }
      if (c < 0) break;
    }
  }
  if (n_tuples == 0) return CP_NO_TUPLE;
  if (n_best == 0) return CP_NO_MAXIMUM;
  for (int c = 0; c < C; ++c) sel[c] = first[c];
  return CP_OK;
}

}  // namespace ia3cp
