// Stand-alone host check of csrc/ia3_cloud.h (the arithmetic cloud.hip runs per source and per axis), built by
// tests/test_clouds_cpu.py with -ffp-contract=off, plain and under AddressSanitizer + UBSan.
//   cloud_cpu <boxes> <terms>
//   boxes: rows of 24 float64: pos[3], h, sig[3], size_fold, shape[3], then NumPy's s (-1: the source is refused),
//          pos_min[3], lo[3], hi[3] and -pos_int + pos of the three axes
//   terms: rows of 8 float64: coord, disp, s, sig, NumPy's u * u, two more terms ta and tb, NumPy's -((ta + tb) + u * u) / 2.
// Prints "boxes <rows> mismatches <rows that differ>", "empty <rows whose box holds no voxel>", "disp mismatches <n>" and
// "terms <rows> mismatches <rows whose term or argument differs in any bit>".
#include <stdio.h>
#include <string.h>
#include <vector>

#include "../../imageanalysis3_amd/csrc/ia3_cloud.h"

using namespace ia3cl;

static bool read_rows(const char* path, int width, std::vector<double>& rows) {
  FILE* f = fopen(path, "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", path); return false; }
  std::vector<double> row(width);
  while (fread(row.data(), sizeof(double), width, f) == (size_t)width) rows.insert(rows.end(), row.begin(), row.end());
  fclose(f);
  return true;
}

static bool same_bits(double a, double b) { return memcmp(&a, &b, sizeof(double)) == 0 || (a != a && b != b); }

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: cloud_cpu <boxes> <terms>\n"); return 2; }
  std::vector<double> boxes, terms;
  if (!read_rows(argv[1], 24, boxes) || !read_rows(argv[2], 8, terms)) return 2;
  long long bad = 0, empty = 0, bad_disp = 0;
  const size_t nb = boxes.size() / 24;
  for (size_t i = 0; i < nb; ++i) {
    const double* r = &boxes[i * 24];
    int s = -1;
    const int refused = cl_size(r[4], r[5], r[6], r[7], &s);
    bool ok = refused ? r[11] == -1.0 : (double)s == r[11];
    if (ok && !refused) {
      const int shape[3] = {(int)r[8], (int)r[9], (int)r[10]};
      ClBox b;
      const bool any = cl_box(r, s, shape, &b);
      bool np_any = true;
      for (int k = 0; k < 3; ++k) {
        np_any = np_any && r[18 + k] > r[15 + k];
        // a source further than CL_POS_MAX away is not worked out: its box is empty, as NumPy's is
        if (r[k] > -CL_POS_MAX && r[k] < CL_POS_MAX)
          ok = ok && (double)b.pmin[k] == r[12 + k] && (double)b.lo[k] == r[15 + k] && (double)b.hi[k] == r[18 + k];
        if (r[k] > -CL_POS_MAX && r[k] < CL_POS_MAX && !same_bits(cl_disp(r[k]), r[21 + k])) ++bad_disp;
      }
      ok = ok && any == np_any;
      if (!any) ++empty;
    }
    if (!ok) {
      if (bad < 5) printf("box row %zu differs\n", i);
      ++bad;
    }
  }
  printf("boxes %zu mismatches %lld\nempty %lld\ndisp mismatches %lld\n", nb, bad, empty, bad_disp);
  long long bad_terms = 0;
  const size_t nt = terms.size() / 8;
  for (size_t i = 0; i < nt; ++i) {
    const double* r = &terms[i * 8];
    const double t = cl_term((long long)r[0], r[1], (int)r[2], r[3]);
    const double a = cl_arg(t, r[5], r[6]);
    if (!same_bits(t, r[4]) || !same_bits(a, r[7])) {
      if (bad_terms < 5) printf("term row %zu: %a and %a, NumPy %a and %a\n", i, t, a, r[4], r[7]);
      ++bad_terms;
    }
  }
  printf("terms %zu mismatches %lld\n", nt, bad_terms);
  printf("pairs %d %d %d\n", cl_pair(0), cl_pair(1), cl_pair(2));
  static_assert(CL_THREADS == 256 && CL_TERMS == 24 && CL_CHUNK == 64, "a tile of four waves, a chunk of one wave");
  return bad || bad_disp || bad_terms ? 1 : 0;
}
