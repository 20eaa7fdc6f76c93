// TEST INFRASTRUCTURE — host build of the index, bit-row and union-find arithmetic of the morphology and labelling kernels
// (csrc/ia3_ccl.h), the header morph.hip compiles for the device: the tile-local unions, the unions across tile faces, the
// numbering of the roots, the word shifts of the erosion / dilation and the run sums of the centres can be compared with
// SciPy and NumPy on the CPU.  Not shipped, not a fallback.
#include "../../imageanalysis3_amd/csrc/ia3_ccl.h"
#include <vector>

using namespace ia3ccl;

// lab = the labelling morph.hip makes of a (Z, X, Y) 0 / non-zero byte mask, by the same steps: union-find per tile,
// unions across the low faces of the tiles, flatten, roots numbered in ascending flat index.  Returns the number of labels.
extern "C" int ia3cpu_label(const unsigned char* mask, int Z, int X, int Y, int* lab) {
  const size_t n = (size_t)Z * X * Y;
  std::vector<int> parent(n, -1);
  int* P = parent.data();
  for (int z0 = 0; z0 < Z; z0 += TZ)
    for (int x0 = 0; x0 < X; x0 += TX)
      for (int y0 = 0; y0 < Y; y0 += TY) {
        int par[TILE];
        for (int i = 0; i < TILE; ++i) {
          int lz, lx, ly;
          tile_coords(i, &lz, &lx, &ly);
          const int z = z0 + lz, x = x0 + lx, y = y0 + ly;
          par[i] = z < Z && x < X && y < Y && mask[((size_t)z * X + x) * Y + y] ? i : -1;
        }
        auto ld = [&par](int i) { return par[i]; };
        auto amin = [&par](int i, int v) { const int old = par[i]; if (v < old) par[i] = v; return old; };
        for (int i = 0; i < TILE; ++i) {
          if (par[i] < 0) continue;
          int lz, lx, ly;
          tile_coords(i, &lz, &lx, &ly);
          if (ly > 0 && par[i - 1] >= 0) unite(ld, amin, i, i - 1);
          if (lx > 0 && par[i - TY] >= 0) unite(ld, amin, i, i - TY);
          if (lz > 0 && par[i - TX * TY] >= 0) unite(ld, amin, i, i - TX * TY);
        }
        for (int i = 0; i < TILE; ++i) {
          if (par[i] < 0) continue;
          int lz, lx, ly, rz, rx, ry;
          tile_coords(i, &lz, &lx, &ly);
          tile_coords(find_root(ld, i), &rz, &rx, &ry);
          P[((size_t)(z0 + lz) * X + x0 + lx) * Y + y0 + ly] = (int)(((size_t)(z0 + rz) * X + x0 + rx) * Y + y0 + ry);
        }
      }
  auto ld = [P](int i) { return P[i]; };
  auto amin = [P](int i, int v) { const int old = P[i]; if (v < old) P[i] = v; return old; };
  // the faces in reverse raster order: the device meets them in no particular order
  for (size_t gg = n; gg-- > 0;) {
    const int g = (int)gg;
    if (P[g] < 0) continue;
    const int y = g % Y, x = (g / Y) % X, z = g / (Y * X);
    if (y % TY == 0 && y > 0 && P[g - 1] >= 0) unite(ld, amin, g, g - 1);
    if (x % TX == 0 && x > 0 && P[g - Y] >= 0) unite(ld, amin, g, g - Y);
    if (z % TZ == 0 && z > 0 && P[g - X * Y] >= 0) unite(ld, amin, g, g - X * Y);
  }
  for (size_t g = 0; g < n; ++g)
    if (P[g] >= 0) P[g] = find_root(ld, (int)g);
  int next = 0;
  for (size_t g = 0; g < n; ++g) lab[g] = P[g] == (int)g ? ++next : 0;
  for (size_t g = 0; g < n; ++g)
    if (P[g] >= 0) lab[g] = lab[P[g]];
  return next;
}

// erosion (dilate = 0) / dilation of a byte mask by ball(r) through the packed rows and word shifts of the kernels
extern "C" void ia3cpu_morph(const unsigned char* mask, int Z, int X, int Y, int r, int dilate, int border, unsigned char* out) {
  const int W = words_per_row(Y);
  std::vector<uint64_t> bits((size_t)Z * X * W, 0), res((size_t)Z * X * W, 0);
  for (size_t row = 0; row < (size_t)Z * X; ++row)
    for (int y = 0; y < Y; ++y)
      if (mask[row * Y + y]) bits[row * W + (y >> 6)] |= 1ull << (y & 63);
  for (int z = 0; z < Z; ++z)
    for (int x = 0; x < X; ++x)
      for (int w = 0; w < W; ++w) res[((size_t)z * X + x) * W + w] = morph_word(bits.data(), Z, X, Y, W, r, dilate, border, z, x, w);
  for (size_t row = 0; row < (size_t)Z * X; ++row)
    for (int y = 0; y < Y; ++y) out[row * Y + y] = (unsigned char)((res[row * W + (y >> 6)] >> (y & 63)) & 1);
}

// out3 = {first offset, last offset, cleared edge width} of a range filter of size s
extern "C" void ia3cpu_window(int s, int* out3) {
  out3[0] = window_lo(s);
  out3[1] = window_hi(s);
  out3[2] = edge_width(s);
}

// ball(r) as a (2 r + 1)^3 byte array
extern "C" void ia3cpu_ball(int r, unsigned char* out) {
  const int w = 2 * r + 1;
  for (int dz = -r; dz <= r; ++dz)
    for (int dx = -r; dx <= r; ++dx)
      for (int dy = -r; dy <= r; ++dy) {
        const int m = ball_reach(r, dz, dx);
        out[((dz + r) * w + dx + r) * w + dy + r] = m >= 0 && dy >= -m && dy <= m;
      }
}

// table: (max_label + 1) x 7 [count, sum z, n(z > 0), sum x, n(x > 0), sum y, n(y > 0)] of an int32 label volume, from
// the runs along y the kernel adds
extern "C" void ia3cpu_label_sums(const int* lab, int Z, int X, int Y, int max_label, unsigned long long* table) {
  for (size_t i = 0; i < ((size_t)max_label + 1) * 7; ++i) table[i] = 0;
  for (int z = 0; z < Z; ++z)
    for (int x = 0; x < X; ++x) {
      const int* row = lab + ((size_t)z * X + x) * Y;
      for (int y = 0; y < Y;) {
        int len = 1;
        while (y + len < Y && row[y + len] == row[y]) ++len;
        if (row[y] > 0 && row[y] <= max_label) {
          unsigned long long add[7];
          run_sums(z, x, y, len, add);
          for (int k = 0; k < 7; ++k) table[(size_t)row[y] * 7 + k] += add[k];
        }
        y += len;
      }
    }
}
