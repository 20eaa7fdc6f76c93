// Stand-alone host check of csrc/ia3_domain.h (the arithmetic domain.hip runs per window and per domain pair), built by
// tests/test_domain_distances_cpu.py with -ffp-contract=off, plain and under AddressSanitizer + UBSan.
//   domain_cpu <windows> <dists>
//   windows: records of float64: R, rows, the R x R distance map, then `rows` times (metric, wd, the R expected values)
//   dists:   records of float64: metric, allow_minus, n_inter, n_intra, expected value, expected integer-0 flag, the inter
//            distances, the intra distances (NaN included)
// The windows go through dm_window_serial; a domain pair goes through the select that dists_k runs, here on one thread:
// histograms of dm_digit over the values that dm_matches, ds_pick_bin, an early end once the rank is alone in its bin, the
// pass that reads the lower middle value off and finds the upper one, dm_nanmedian, dm_dev2 and dm_dist_final.
// Prints "windows <values> mismatches <n>" and "dists <records> mismatches <n>".
#include <stdio.h>
#include <string.h>
#include <vector>

#include "../../imageanalysis3_amd/csrc/ia3_domain.h"

using namespace ia3dm;

static bool read_all(const char* path, std::vector<double>& v) {
  FILE* f = fopen(path, "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", path); return false; }
  double buf[4096];
  size_t n;
  while ((n = fread(buf, sizeof(double), 4096, f)) > 0) v.insert(v.end(), buf, buf + n);
  fclose(f);
  return true;
}

static bool same_bits(double a, double b) { return memcmp(&a, &b, sizeof(double)) == 0 || (a != a && b != b); }

// np.nanmedian of val(v[i]) by the select of dists_k; *count: the values that are not NaN
template <class V>
static double select_median(const std::vector<double>& v, V val, unsigned* count) {
  u64 prefix = 0;
  unsigned k = 0, c = 0;
  int last = DM_PASSES - 1;
  for (int pass = 0; pass < DM_PASSES; ++pass) {
    unsigned hist[DM_BINS] = {0};
    for (double d : v) {
      const double x = val(d);
      if (x != x) continue;
      const u64 key = dm_key(x);
      if (dm_matches(key, prefix, pass)) ++hist[dm_digit(key, pass)];
    }
    if (pass == 0) {
      for (int b = 0; b < DM_BINS; ++b) c += hist[b];
      k = c ? (c - 1) / 2 : 0;
    }
    if (!c) break;
    const int b = ia3ds::ds_pick_bin(hist, 0, DM_BINS, k);
    prefix |= (u64)b << dm_shift(pass);
    if (hist[b] <= 1) { last = pass; break; }
  }
  const int low = dm_shift(last);
  const u64 lo_top = prefix >> low;
  unsigned le = 0;
  u64 mn = ~0ull, lo = 0;
  for (double d : v) {
    const double x = val(d);
    if (x != x) continue;
    const u64 key = dm_key(x), top = key >> low;
    if (top <= lo_top) {
      ++le;
      if (top == lo_top && key > lo) lo = key;
    } else if (key < mn) mn = key;
  }
  *count = c;
  return dm_nanmedian(c, lo, le, mn);
}

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: domain_cpu <windows> <dists>\n"); return 2; }
  std::vector<double> w, d;
  if (!read_all(argv[1], w) || !read_all(argv[2], d)) return 2;
  long long n_win = 0, bad_win = 0;
  std::vector<double> intra(DM_MAX_INTRA), inter(DM_MAX_INTER);
  for (size_t at = 0; at + 2 <= w.size();) {
    const int R = (int)w[at], rows = (int)w[at + 1];
    const double* mat = &w[at + 2];
    at += 2 + (size_t)R * R;
    for (int row = 0; row < rows; ++row) {
      if (at + 2 + R > w.size()) { fprintf(stderr, "windows: a record ends early\n"); return 2; }
      const int metric = (int)w[at], wd = (int)w[at + 1];
      for (int i = 0; i < R; ++i) {
        const double got = dm_window_serial([&](int r, int c) { return mat[(size_t)r * R + c]; }, R, i, wd, metric, intra.data(), inter.data());
        ++n_win;
        if (!same_bits(got, w[at + 2 + i])) {
          if (bad_win < 5) printf("window R %d metric %d wd %d locus %d: %a, expected %a\n", R, metric, wd, i, got, w[at + 2 + i]);
          ++bad_win;
        }
      }
      at += 2 + R;
    }
  }
  printf("windows %lld mismatches %lld\n", n_win, bad_win);
  long long n_dist = 0, bad_dist = 0;
  for (size_t at = 0; at + 6 <= d.size();) {
    const int metric = (int)d[at], allow = (int)d[at + 1];
    const size_t n_inter = (size_t)d[at + 2], n_intra = (size_t)d[at + 3];
    if (at + 6 + n_inter + n_intra > d.size()) { fprintf(stderr, "dists: a record ends early\n"); return 2; }
    const std::vector<double> a(d.begin() + at + 6, d.begin() + at + 6 + n_inter);
    const std::vector<double> b(d.begin() + at + 6 + n_inter, d.begin() + at + 6 + n_inter + n_intra);
    unsigned c_inter, c_intra, c2;
    const double m_inter = select_median(a, [](double x) { return x; }, &c_inter);
    const double m_intra = select_median(b, [](double x) { return x; }, &c_intra);
    double v_inter = 0.0, v_intra = 0.0;
    if (metric == DM_D_MEDIAN && c_inter && c_intra) {
      v_inter = select_median(a, [&](double x) { return dm_dev2(x, m_inter); }, &c2);
      v_intra = select_median(b, [&](double x) { return dm_dev2(x, m_intra); }, &c2);
    }
    int zero = 0;
    const double got = dm_dist_final(metric, c_inter, c_intra, m_inter, m_intra, v_inter, v_intra, allow, &zero);
    ++n_dist;
    if (!same_bits(got, d[at + 4]) || zero != (int)d[at + 5]) {
      if (bad_dist < 5) printf("dist record %lld: %a (%d), expected %a (%d)\n", n_dist - 1, got, zero, d[at + 4], (int)d[at + 5]);
      ++bad_dist;
    }
    at += 6 + n_inter + n_intra;
  }
  printf("dists %lld mismatches %lld\n", n_dist, bad_dist);
  static_assert(DM_MAX_INTRA == 240 && DM_MAX_INTER == 256 && DM_PASSES * DM_DIGIT == 64, "the sets of a window of 16; all 64 key bits");
  return bad_win || bad_dist ? 1 : 0;
}
