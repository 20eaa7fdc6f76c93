// Stand-alone host check of csrc/ia3_density.h (the arithmetic density.hip runs per pair), built by
// tests/test_compartment_density_cpu.py with -ffp-contract=off, plain and under AddressSanitizer + UBSan.
//   density_cpu <file>   file: rows of ten float64 (contributor z x y, query z x y, squared sigmas z x y, NumPy's t)
// Prints "args <rows> mismatches <rows whose dn_arg differs from t in any bit>", the weight of every (flags, same copy,
// self, multiplicity) as "w <flags> <same> <self> <mult> <weight>", and "pack <words checked> <bad>".
#include <stdio.h>
#include <string.h>
#include <vector>

#include "../../imageanalysis3_amd/csrc/ia3_density.h"

using namespace ia3dn;

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: density_cpu <file>\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  std::vector<double> rows;
  double row[10];
  while (fread(row, sizeof(double), 10, f) == 10) rows.insert(rows.end(), row, row + 10);
  fclose(f);
  long long bad = 0;
  const size_t n = rows.size() / 10;
  for (size_t i = 0; i < n; ++i) {
    const double* r = &rows[i * 10];
    const double t = dn_arg(r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], r[8]);
    if (memcmp(&t, &r[9], sizeof(double)) != 0 && !(t != t && r[9] != r[9])) {
      if (bad < 5) printf("row %zu: %a, NumPy %a\n", i, t, r[9]);
      ++bad;
    }
    // the sign of the difference does not reach the square
    const double u = dn_arg(r[3], r[4], r[5], r[0], r[1], r[2], r[6], r[7], r[8]);
    if (memcmp(&t, &u, sizeof(double)) != 0 && !(t != t && u != u)) ++bad;
  }
  printf("args %zu mismatches %lld\n", n, bad);
  for (int flags = 0; flags < 8; ++flags)
    for (int same = 0; same < 2; ++same)
      for (int self = 0; self < 2; ++self)
        for (int mult : {0, 1, 3}) printf("w %d %d %d %d %d\n", flags, same, self, mult, dn_weight(same != 0, self != 0, mult, flags));
  long long words = 0, bad_words = 0;
  for (int copy : {0, 1, 255, 256, 65535})
    for (int a : {0, 1, 128, 255})
      for (int b : {0, 1, 128, 255}) {
        const uint32_t w = dn_pack(copy, a, b);
        ++words;
        if (dn_copy(w) != copy || dn_mult_a(w) != a || dn_mult_b(w) != b || ((w >> 16) == 0) != (a == 0 && b == 0)) ++bad_words;
      }
  printf("pack %lld %lld\n", words, bad_words);
  static_assert(DN_CELL_MAX == 65536 && DN_CTILE % DN_PART == 0 && DN_PART == 64, "the cap of a copy number and the parts of a sum");
  return bad || bad_words ? 1 : 0;
}
