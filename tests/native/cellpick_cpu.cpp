// Stand-alone host check of csrc/ia3_cellpick.h: the serial text that cellpick.hip runs per lane, on records that
// tests/test_cell_picking_cpu.py writes from tests/golden/cell_picking.npz (the reference's merged lists, and the scores,
// dynamic scores, pointers and picked indices its dynamic picker held).  A record is a run of float64 values:
//   1, C, has_coords, has_th, th, hard, dist_th, R, coords (3 C); per region: the C list lengths, the rows (n, 4), their
//      NaN flags (n); then the expected K, its valid count and merged rows (K, 4)
//   2, C, share, kind, w, hi, nan_mask, nv, dzxy (3), K (nv), gaps (nv), rows (sum K, 4), scores (C, sum K); per chromosome
//      the reference distance (linear) or n, the sorted values (n) and the table (n + 1); then the expected dynamic scores
//      (C, sum K), pointers (C, sum K; -1 none) and picked indices (C, nv)
// Prints "regions <n> rows <n> steps <n> spots <n> mismatches <n>".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "../../imageanalysis3_amd/csrc/ia3_cellpick.h"

using namespace ia3cp;

static bool same(double a, double b) {
  if (a != a || b != b) return (a != a) == (b != b);
  return memcmp(&a, &b, sizeof(double)) == 0;
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: cellpick_cpu records.bin\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror("open"); return 2; }
  fseek(f, 0, SEEK_END);
  const long bytes = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<double> rec((size_t)bytes / sizeof(double));
  if (fread(rec.data(), sizeof(double), rec.size(), f) != rec.size()) { fprintf(stderr, "short read\n"); return 2; }
  fclose(f);
  size_t at = 0;
  auto take = [&](size_t n) { const double* p = rec.data() + at; at += n; if (at > rec.size()) { fprintf(stderr, "record overrun\n"); exit(2); } return p; };
  long regions = 0, rows_checked = 0, steps = 0, spots = 0, bad = 0;
  {  // the walk is bounded: 64^3 tuples run, 64^4 are refused
    int na[4] = {64, 64, 64, 64}, sel[4];
    auto idx = [](int, int a) { return a; };
    auto meas = [](int c, int p) { return (double)(c + p); };
    if (cp_pick(3, 64, na, idx, meas, true, sel) != CP_OK || sel[0] != 63 || sel[2] != 63) ++bad;
    if (cp_pick(4, 64, na, idx, meas, true, sel) != CP_TOO_MANY) ++bad;
  }
  while (at < rec.size()) {
    const int type = (int)*take(1);
    if (type == 1) {
      const double* hd = take(7);
      const int C = (int)hd[0], has_coords = (int)hd[1], has_th = (int)hd[2], hard = (int)hd[4], R = (int)hd[6];
      const double th = hd[3], dist_th = hd[5];
      const double* coords = take((size_t)3 * C);
      for (int r = 0; r < R; ++r) {
        const double* len = take((size_t)C);
        int start[CP_MAX_CHROM + 1] = {0};
        for (int c = 0; c < C; ++c) start[c + 1] = start[c] + (int)len[c];
        const int n = start[C];
        const double* rows = take((size_t)4 * n);
        const double* nanf = take((size_t)n);
        std::vector<unsigned char> row_nan((size_t)n + 1), keep((size_t)n + C + 1);
        for (int i = 0; i < n; ++i) row_nan[i] = nanf[i] != 0.0;
        std::vector<int> src((size_t)n + 2 * C + 1);
        std::vector<double> out(4 * ((size_t)n + 2 * C + 1));
        MergeList L;
        L.rows = rows; L.start = start; L.coords = has_coords ? coords : nullptr; L.C = C;
        int valid = 0;
        const int K = cp_merge_region(L, row_nan.data(), has_th, th, hard, dist_th, keep.data(), src.data(), out.data(), &valid);
        const int wantK = (int)*take(1), want_valid = (int)*take(1);
        const double* want = take((size_t)4 * wantK);
        ++regions;
        if (K != wantK || valid != want_valid) { ++bad; continue; }
        for (int i = 0; i < 4 * K; ++i) { ++rows_checked; if (!same(out[i], want[i])) ++bad; }
      }
    } else if (type == 2) {
      const double* hd = take(7);
      const int C = (int)hd[0], share = (int)hd[1], kind = (int)hd[2], nv = (int)hd[6];
      const double w = hd[3], hi = hd[4], nan_mask = hd[5];
      const double* dz = take(3);
      const double* Kd = take((size_t)nv);
      const double* gaps = take((size_t)nv);
      std::vector<int> K(nv), b(nv + 1, 0);
      for (int i = 0; i < nv; ++i) { K[i] = (int)Kd[i]; b[i + 1] = b[i] + K[i]; }
      const int N = b[nv];
      const double* rows = take((size_t)4 * N);
      const double* sc = take((size_t)C * N);
      std::vector<double> dy(sc, sc + (size_t)C * N);
      std::vector<int> ptr((size_t)C * N, -1);
      NbRef refs[CP_MAX_CHROM];
      for (int c = 0; c < C; ++c) {
        NbRef& r = refs[c];
        r.kind = kind; r.w = w; r.hi = hi; r.nan_mask = nan_mask; r.ref = 0.0; r.sorted = nullptr; r.table = nullptr; r.n = 0;
        if (kind == ia3sc::SC_DIST_LINEAR) r.ref = *take(1);
        else { r.n = (int)*take(1); r.sorted = take((size_t)r.n); r.table = take((size_t)r.n + 1); }
      }
      std::vector<double> dist((size_t)CP_MAX_SPOTS * CP_MAX_SPOTS);
      int err = 0;
      for (int s = 0; s + 1 < nv; ++s) {
        const int K0 = K[s], K1 = K[s + 1], b0 = b[s], b1 = b[s + 1];
        const long long gap = (long long)gaps[s + 1];
        for (int n = 0; n < K1; ++n) {
          const double* m = rows + 4 * (size_t)(b1 + n);
          const double z = m[1] * dz[0], x = m[2] * dz[1], y = m[3] * dz[2];
          for (int p = 0; p < K0; ++p) {
            const double* q = rows + 4 * (size_t)(b0 + p);
            dist[(size_t)p * CP_MAX_SPOTS + n] = ia3sc::sc_norm_rows(q[1] * dz[0] - z, q[2] * dz[1] - x, q[3] * dz[2] - y);
          }
        }
        int allowed[CP_MAX_CHROM][CP_MAX_SPOTS], na[CP_MAX_CHROM];
        for (int c = 0; c < C; ++c) {
          const double* d = dy.data() + (size_t)c * N + b0;
          na[c] = cp_allowed([&](int p) { return d[p]; }, K0, C, allowed[c]);
        }
        for (int n = 0; n < K1; ++n) {
          auto meas = [&](int c, int p) { return cp_measure(refs[c], dist[(size_t)p * CP_MAX_SPOTS + n], gap, dy[(size_t)c * N + b0 + p]); };
          int sel[CP_MAX_CHROM];
          const int rc = cp_pick(C, K0, na, [&](int c, int a) { return allowed[c][a]; }, meas, share != 0, sel);
          if (rc != CP_OK) { err = rc; continue; }
          for (int c = 0; c < C; ++c) {
            dy[(size_t)c * N + b1 + n] += meas(c, sel[c]);
            ptr[(size_t)c * N + b1 + n] = sel[c];
          }
          ++spots;
        }
        ++steps;
      }
      const double* want_dy = take((size_t)C * N);
      const double* want_ptr = take((size_t)C * N);
      const double* want_idx = take((size_t)C * nv);
      if (err) ++bad;
      for (size_t i = 0; i < (size_t)C * N; ++i) {
        if (!same(dy[i], want_dy[i])) ++bad;
        if (ptr[i] != (int)want_ptr[i]) ++bad;
      }
      // backward (:1158-1169): np.argmax of the last dynamic scores, then the pointers
      for (int c = 0; c < C && nv > 0; ++c) {
        const double* last = dy.data() + (size_t)c * N + b[nv - 1];
        int idx = 0;
        for (int k = 1; k < K[nv - 1]; ++k)
          if (last[idx] == last[idx] && (last[k] > last[idx] || last[k] != last[k])) idx = k;
        for (int s = nv - 1; s >= 0; --s) {
          if (idx != (int)want_idx[(size_t)c * nv + s]) ++bad;
          if (s > 0) idx = ptr[(size_t)c * N + b[s] + idx];
          if (idx < 0) { ++bad; break; }
        }
      }
    } else {
      fprintf(stderr, "unknown record %d at %zu\n", type, at);
      return 2;
    }
  }
  printf("regions %ld rows %ld steps %ld spots %ld mismatches %ld\n", regions, rows_checked, steps, spots, bad);
  return bad ? 1 : 0;
}
