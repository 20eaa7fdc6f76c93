// Stand-alone host check of csrc/ia3_score.h and of np_sum_any (csrc/ia3_npsum.h): the serial text score.hip runs per lane,
// built by tests/test_scoring_cpu.py with -ffp-contract=off, plain and under AddressSanitizer + UBSan.
//   score_cpu <records>
// records: float64 values, a sequence of
//   1, N, a[N], expected[N]                       expected[n - 1] = np.add.reduce(a[:n])
//   2, n_cand, n_sel, has_center, centre[3] (pixels), distance_zxy[3], intensity_th, candidate rows (4 each), candidate
//      ids, selected rows, selected ids, then until a 0:
//        10, ct[n_cand]                           _center_distance of the candidates (centre given, or their own mean)
//        11, half, lc[n_cand]                     _local_distance against the selected rows
//        12, fwd[n_cand], rev[n_cand]             neighboring_distances among the candidates
//        13, metric, ignore_nan, len[4], values   generate_ref_from_chromosome of the selected rows (len -1: not compared)
//   3, kind, n_ref, n_x, w, lo, hi, ref_scalar, nan_mask, ref[n_ref], x[n_x], expected[n_x]     sc_score without np.log
// Prints "sums <n> geometry <n> references <n> values <n> mismatches <n>".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>

#include "../../imageanalysis3_amd/csrc/ia3_score.h"

using namespace ia3sc;

static bool same_bits(double a, double b) { return memcmp(&a, &b, sizeof(double)) == 0 || (a != a && b != b); }

struct HostTable {
  std::vector<double> rows;
  std::vector<int> id, sid, perm;
  void index() {
    const int n = (int)id.size();
    perm.resize(n);
    for (int i = 0; i < n; ++i) perm[i] = i;
    std::stable_sort(perm.begin(), perm.end(), [&](int a, int b) { return id[a] < id[b]; });
    sid.resize(n);
    for (int i = 0; i < n; ++i) sid[i] = id[perm[i]];
  }
  RowIndex view(const double* dz) const {
    RowIndex r;
    r.rows = rows.data(); r.sid = sid.data(); r.perm = perm.data(); r.dzxy = dz; r.lo = 0; r.hi = (int)id.size();
    return r;
  }
};

static void mean_of(const HostTable& t, const double* dz, double* m) {
  Mean3 mean;
  for (size_t i = 0; i < t.id.size(); ++i) {
    double v[3];
    sc_zxy(t.rows.data() + 4 * i, dz, v);
    mean.add(v);
  }
  mean.finish(m);
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: score_cpu <records>\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  std::vector<double> d;
  double buf[4096];
  size_t got;
  while ((got = fread(buf, sizeof(double), 4096, f)) > 0) d.insert(d.end(), buf, buf + got);
  fclose(f);
  long n_sum = 0, n_geo = 0, n_ref = 0, n_val = 0, bad = 0;
  size_t at = 0;
  auto need = [&](size_t k) { if (at + k > d.size()) { fprintf(stderr, "truncated records at %zu\n", at); exit(2); } };
  auto miss = [&](const char* what, long i, double a, double b) {
    if (++bad <= 20) fprintf(stderr, "%s[%ld]: %.17g, expected %.17g\n", what, i, a, b);
  };
  while (at < d.size()) {
    const int tag = (int)d[at++];
    if (tag == 1) {
      need(1);
      const int N = (int)d[at++];
      need(2 * (size_t)N);
      const double* a = d.data() + at;
      const double* want = a + N;
      for (int n = 1; n <= N; ++n) {
        const double s = ia3::np_sum_any<double>([a](int i) { return a[i]; }, n);
        if (!same_bits(s, want[n - 1])) miss("sum", n, s, want[n - 1]);
        if (n <= ia3::NPSUM_MAX && !same_bits(ia3::np_sum(a, n), s)) miss("sum512", n, ia3::np_sum(a, n), s);
        ++n_sum;
      }
      at += 2 * (size_t)N;
    } else if (tag == 2) {
      need(10);
      const int nc = (int)d[at], ns = (int)d[at + 1], has_center = (int)d[at + 2];
      const double* cpx = d.data() + at + 3;
      double dz[3] = {d[at + 6], d[at + 7], d[at + 8]};
      const double th = d[at + 9];
      at += 10;
      need(5 * (size_t)(nc + ns));
      HostTable cand, sel;
      cand.rows.assign(d.begin() + at, d.begin() + at + 4 * nc); at += 4 * (size_t)nc;
      for (int i = 0; i < nc; ++i) cand.id.push_back((int)d[at++]);
      sel.rows.assign(d.begin() + at, d.begin() + at + 4 * ns); at += 4 * (size_t)ns;
      for (int i = 0; i < ns; ++i) sel.id.push_back((int)d[at++]);
      cand.index();
      sel.index();
      const RowIndex ci = cand.view(dz), si = sel.view(dz);
      double given[3], cmean[3], smean[3];
      for (int k = 0; k < 3; ++k) given[k] = cpx[k] * dz[k];
      mean_of(cand, dz, cmean);
      mean_of(sel, dz, smean);
      for (;;) {
        need(1);
        const int sub = (int)d[at++];
        if (sub == 0) break;
        if (sub == 10) {
          need(nc);
          const double* ctr = has_center ? given : cmean;
          for (int i = 0; i < nc; ++i, ++n_geo) {
            double t[3];
            sc_zxy(cand.rows.data() + 4 * (size_t)i, dz, t);
            const double v = sc_norm_rows(t[0] - ctr[0], t[1] - ctr[1], t[2] - ctr[2]);
            if (!same_bits(v, d[at + i])) miss("ct", i, v, d[at + i]);
          }
          at += nc;
        } else if (sub == 11) {
          need(1 + (size_t)nc);
          const int half = (int)d[at++];
          for (int i = 0; i < nc; ++i, ++n_geo) {
            double t[3];
            sc_zxy(cand.rows.data() + 4 * (size_t)i, dz, t);
            const double v = sc_local(t, cand.id[i], half, sc_nan(), si);
            if (!same_bits(v, d[at + i])) miss("lc", i, v, d[at + i]);
          }
          at += nc;
        } else if (sub == 12) {
          need(2 * (size_t)nc);
          for (int i = 0; i < nc; ++i, ++n_geo) {
            double t[3], fwd, rev;
            sc_zxy(cand.rows.data() + 4 * (size_t)i, dz, t);
            sc_neighbors(t, cand.id[i], 1, sc_nan(), ci, &fwd, &rev);
            if (!same_bits(fwd, d[at + i])) miss("fwd", i, fwd, d[at + i]);
            if (!same_bits(rev, d[at + nc + i])) miss("rev", i, rev, d[at + nc + i]);
          }
          at += 2 * (size_t)nc;
        } else if (sub == 13) {
          need(6);
          const int metric = (int)d[at], ign = (int)d[at + 1];
          int len[4];
          for (int a = 0; a < 4; ++a) len[a] = (int)d[at + 2 + a];
          at += 6;
          const double* ctr = has_center ? given : smean;
          std::vector<double> raw[4];
          for (int i = 0; i < ns; ++i) {
            double t[3], fwd, rev;
            const double* row = sel.rows.data() + 4 * (size_t)i;
            sc_zxy(row, dz, t);
            raw[0].push_back(sc_norm_rows(t[0] - ctr[0], t[1] - ctr[1], t[2] - ctr[2]));
            raw[1].push_back(sc_local(t, sel.id[i], 2, sc_nan(), si));
            sc_neighbors(t, sel.id[i], 1, sc_nan(), si, &fwd, &rev);
            raw[2].push_back(fwd);
            raw[3].push_back(row[0] <= th ? sc_nan() : row[0]);
          }
          const double fallback[4] = {1000.0, sc_inf(), sc_inf(), 1.0};
          for (int a = 0; a < 4; ++a) {
            std::vector<double> comp;
            for (double v : raw[a]) if (!ign || v == v) comp.push_back(v);
            if (ign && comp.empty()) comp.push_back(fallback[a]);
            std::vector<double> sorted;
            for (double v : comp) if (v == v) sorted.push_back(v);
            std::sort(sorted.begin(), sorted.end());
            std::vector<double> out;
            if (metric == SC_REF_MEDIAN) out.push_back(sc_median_sorted(sorted.data(), (int)sorted.size()));
            else if (metric == SC_REF_MEAN) out.push_back(sc_nanmean_1d([&](int i) { return comp[i]; }, (int)comp.size()));
            else if (metric == SC_REF_RG && a < 3)
              out.push_back(sc_rg([&](int i, double* v) { sc_zxy(sel.rows.data() + 4 * (size_t)i, dz, v); }, ns, smean));
            else out = comp;
            if (len[a] >= 0) {
              need((size_t)len[a]);
              if ((int)out.size() != len[a]) { miss("ref length", a, (double)out.size(), (double)len[a]); }
              else for (int i = 0; i < len[a]; ++i, ++n_ref) if (!same_bits(out[i], d[at + i])) miss("ref", a * 1000 + i, out[i], d[at + i]);
              at += (size_t)len[a];
            }
          }
        } else { fprintf(stderr, "unknown sub-record %d\n", sub); return 2; }
      }
    } else if (tag == 3) {
      need(8);
      const int kind = (int)d[at], nr = (int)d[at + 1], nx = (int)d[at + 2];
      const double w = d[at + 3], lo = d[at + 4], hi = d[at + 5], ref_scalar = d[at + 6], nan_mask = d[at + 7];
      at += 8;
      need((size_t)nr + 2 * (size_t)nx);
      std::vector<double> sorted;
      for (int i = 0; i < nr; ++i) if (d[at + i] == d[at + i]) sorted.push_back(d[at + i]);
      std::sort(sorted.begin(), sorted.end());
      at += nr;
      for (int i = 0; i < nx; ++i, ++n_val) {
        int cls;
        double v = sc_score(kind, d[at + i], ref_scalar, sorted.data(), (int)sorted.size(), w, lo, hi, &cls);
        if (kind == SC_DIST_LINEAR && (cls & SC_NAN_IN)) v = nan_mask;
        if ((cls & 3) != SC_VALUE) miss("class", i, cls, 0);
        if (!same_bits(v, d[at + nx + i])) miss("value", i, v, d[at + nx + i]);
      }
      at += 2 * (size_t)nx;
    } else { fprintf(stderr, "unknown record %d at %zu\n", tag, at); return 2; }
  }
  printf("sums %ld geometry %ld references %ld values %ld mismatches %ld\n", n_sum, n_geo, n_ref, n_val, bad);
  return bad ? 1 : 0;
}
