// Index, bit-row and union-find arithmetic of the binary morphology and of the connected-component labelling
// (morph.hip).  Compiles for the device and for the host: tests/native/ccl_cpu.cpp builds the same
// functions into a CPU labelling that is compared with scipy.ndimage.label.
#pragma once
#include <stdint.h>
#include <stddef.h>

#if defined(__HIPCC__)
#define IA3_CCL_HD __host__ __device__ inline
#else
#define IA3_CCL_HD inline
#endif

namespace ia3ccl {

// ---- tiles of the labelling --------------------------------------------------------------------------------------------
constexpr int TZ = 4, TX = 8, TY = 32;          // voxels of one LDS tile along z, x, y
constexpr int TILE = TZ * TX * TY;              // 1024
// local raster index inside a tile; the raster order of two voxels of one tile is that of their flat indices in the stack
IA3_CCL_HD int tile_index(int lz, int lx, int ly) { return (lz * TX + lx) * TY + ly; }
IA3_CCL_HD void tile_coords(int i, int* lz, int* lx, int* ly) {
  *ly = i % TY;
  *lx = (i / TY) % TX;
  *lz = i / (TY * TX);
}
IA3_CCL_HD int tiles(int n, int t) { return (n + t - 1) / t; }

// ---- bit rows ------------------------------------------------------------------------------------------------------------
// A mask is one bit per voxel, bit y & 63 of word y >> 6 of its row; every row takes words_per_row(Y) 64-bit words and the
// bits past Y are zero.
IA3_CCL_HD int words_per_row(int Y) { return (Y + 63) >> 6; }
IA3_CCL_HD uint64_t valid_bits(int Y, int w) {   // the bits of word w that are voxels
  const int left = Y - (w << 6);
  return left >= 64 ? ~0ull : (left <= 0 ? 0ull : (~0ull >> (64 - left)));
}
// bit y of the result = bit y + k of the row around word `cur` (k = -2..2)
IA3_CCL_HD uint64_t shift_y(uint64_t prev, uint64_t cur, uint64_t next, int k) {
  if (k == 0) return cur;
  if (k > 0) return (cur >> k) | (next << (64 - k));
  return (cur << -k) | (prev >> (64 + k));
}
// skimage.morphology.ball(r): offsets with dz^2 + dx^2 + dy^2 <= r^2.  The largest |dy| of the ball at (dz, dx), or -1
// where the ball has no voxel (r = 0..2).
IA3_CCL_HD int ball_reach(int r, int dz, int dx) {
  const int rem = r * r - dz * dz - dx * dx;
  if (rem < 0) return -1;
  return rem >= 4 ? 2 : (rem >= 1 ? 1 : 0);
}

// word w of a row as an operator reads it: rows, words and bits outside the volume count as `fill` (all ones or zero)
IA3_CCL_HD uint64_t row_word(const uint64_t* row, int w, int W, int Y, uint64_t fill) {
  if (w < 0 || w >= W) return fill;
  const uint64_t valid = valid_bits(Y, w);
  return (row[w] & valid) | (fill & ~valid);
}
// Word (z, x, w) of the erosion (dilate = 0) or dilation of `in` by ball(r): for every (dz, dx) of the ball the row's word
// and its two neighbours are shifted by each dy the ball reaches there, and the shifted words are ANDed (ORed).  The ball
// is symmetric, so no reflection is needed.  border: what the outside of the volume counts as.
IA3_CCL_HD uint64_t morph_word(const uint64_t* in, int Z, int X, int Y, int W, int r, int dilate, int border, int z, int x,
                               int w) {
  const uint64_t fill = border ? ~0ull : 0ull;
  uint64_t acc = dilate ? 0ull : ~0ull;
  for (int dz = -r; dz <= r; ++dz)
    for (int dx = -r; dx <= r; ++dx) {
      const int m = ball_reach(r, dz, dx);
      if (m < 0) continue;
      const int zz = z + dz, xx = x + dx;
      uint64_t prev = fill, cur = fill, next = fill;
      if (zz >= 0 && zz < Z && xx >= 0 && xx < X) {
        const uint64_t* rp = in + ((size_t)zz * X + xx) * (size_t)W;
        cur = row_word(rp, w, W, Y, fill);
        if (m > 0) { prev = row_word(rp, w - 1, W, Y, fill); next = row_word(rp, w + 1, W, Y, fill); }
      }
      for (int k = -m; k <= m; ++k) {
        const uint64_t sft = shift_y(prev, cur, next, k);
        acc = dilate ? (acc | sft) : (acc & sft);
      }
    }
  return acc & valid_bits(Y, w);
}

// ---- the range filter's window and the cleared edge ------------------------------------------------------------------------
// scipy.ndimage.maximum_filter(size=s): offsets -(s / 2) .. s - 1 - s / 2 along every axis (s = 4: -2 .. +1)
IA3_CCL_HD int window_lo(int s) { return -(s / 2); }
IA3_CCL_HD int window_hi(int s) { return s - 1 - s / 2; }
IA3_CCL_HD int edge_width(int s) { return (s + 1) / 2; }   // int(np.ceil(s / 2))
IA3_CCL_HD int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---- union-find ------------------------------------------------------------------------------------------------------------
// parent[i] <= i always, so a walk to the root visits strictly decreasing indices and ends; the root of a tree is its
// smallest member.  `ld(i)` reads parent[i]; `amin(i, v)` does parent[i] = min(parent[i], v) atomically and returns the old
// value.  A read that is out of date only starts the walk further from the root: every value parent[i] ever held is a
// member of i's component that is no larger than i.
template <class Load>
IA3_CCL_HD int find_root(Load ld, int i) {
  for (;;) {
    const int p = ld(i);
    if (p == i) return i;
    i = p;
  }
}
// Joins the trees of a and b: the larger root is hung below the smaller one.  When another thread re-hung that root in
// the meantime (old != a), the three trees involved still have to become one, so the work goes on with (old, b): both
// smaller than a, which bounds the loop.
template <class Load, class AMin>
IA3_CCL_HD void unite(Load ld, AMin amin, int a, int b) {
  for (;;) {
    a = find_root(ld, a);
    b = find_root(ld, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = amin(a, b);
    if (old == a) return;
    a = old;
  }
}

// ---- centres -----------------------------------------------------------------------------------------------------------------
// A run of `len` voxels of one label along y, from y0, in row (z, x): what it adds to the label's row
// [count, sum z, n(z > 0), sum x, n(x > 0), sum y, n(y > 0)] (segmentation_tools/chromosome.py:4-10 averages, per axis,
// the indices > 0 only)
IA3_CCL_HD void run_sums(int z, int x, int y0, int len, unsigned long long* add7) {
  const unsigned long long l = (unsigned long long)len;
  add7[0] = l;
  add7[1] = (unsigned long long)z * l;
  add7[2] = z > 0 ? l : 0;
  add7[3] = (unsigned long long)x * l;
  add7[4] = x > 0 ? l : 0;
  add7[5] = ((unsigned long long)y0 + (unsigned long long)(y0 + len - 1)) * l / 2;
  add7[6] = y0 > 0 ? l : l - 1;
}

}  // namespace ia3ccl
