// Host side of the column-in-registers axis-0 kernel (gauss_col_kernel.inc): its weight stream and the default guard of
// its certificate, stated once for the built depths (gauss_col.inc) and the run-time compiled ones (gauss_col_dispatch.hip).
#pragma once
#include <vector>

#include "ia3_gauss_dev.h"

namespace ia3g {

// The even/odd weight stream of depth Z, radius R (taps w[0 .. R], symmetric) and border mode.  W[z][p] = the taps of
// output z that land on plane p, added up in f64 in tap order -R .. R as before; then, with H = Z / 2,
//   Wp[z][q] = (W[z][q] + W[z][Z-1-q]) / 2,  Wm[z][q] = (W[z][q] - W[z][Z-1-q]) / 2   (q < H; the halving is exact).
// Stream: rows z = 0 .. H-1, each Wp[z][0], Wm[z][0], Wp[z][1], Wm[z][1], ... (the two chains of the kernel advance
// together, so every piece of the stream feeds both), then for an odd depth the centre plane's own weight W[z][H]; an odd
// depth ends with the centre row z = H: Wp[H][0 .. H-1] = W[H][q] (its Wm is zero by symmetry) and W[H][H].  That is
// Z per row, Z * Z / 2 doubles in all (+ (Z+1)/2 for an odd depth), padded with zeros to a multiple of 16.
inline std::vector<double> col_evenodd_rows(int Z, int R, int mode, const double* w) {
  const int H = Z / 2;
  std::vector<double> W((size_t)Z), rows;
  for (int z = 0; z < (Z + 1) / 2; ++z) {
    for (int p = 0; p < Z; ++p) {
      double acc = 0.0;
      for (int j = -R; j <= R; ++j)
        if (border_idx(z + j, Z, mode) == p) acc += w[j < 0 ? -j : j];
      W[p] = acc;
    }
    for (int q = 0; q < H; ++q) {
      rows.push_back((W[q] + W[Z - 1 - q]) * 0.5);
      if (z < H) rows.push_back((W[q] - W[Z - 1 - q]) * 0.5);
    }
    if (Z & 1) rows.push_back(W[H]);
  }
  rows.resize((rows.size() + 15) / 16 * 16, 0.0);
  return rows;
}

// K of the kernel's rule (i): a mirror pair whose smaller output is below P / K takes the reference sequence
constexpr int COL_LOPSIDED_K = 4;

// Default guard of the even/odd sum, in f64 ulps of the output (the derivation is in the kernel's header comment):
//   K * (2 n + 2 tw + 6) + 3 R + 4,   n = (Z+1)/2 terms per chain, tw = roundings in one W[z][p]
// tw: 'nearest' piles up to R + 1 taps on a border plane (R additions); 'reflect' has period 2 Z, a plane is met at most
// twice per period, and the 2 R + 1 taps span ceil((2R+1) / (2Z)) periods.
inline int col_guard(int Z, int R, int mode) {
  const int n = (Z + 1) / 2;
  const int tw = mode == IA3_MODE_NEAREST ? R : 2 * ((2 * R + 1 + 2 * Z - 1) / (2 * Z)) - 1;
  return COL_LOPSIDED_K * (2 * n + 2 * tw + 6) + 3 * R + 4;
}

}  // namespace ia3g
