// Index arithmetic of the label lookups (labels.hip), shared with the host build tests/native/labels_cpu.cpp: how a spot
// centre becomes a voxel, the order of the (2r+1)^3 offsets around it and how an offset that leaves the image is
// brought back.  Reference: classes/partition_spots.py:212-236 find_coordinate_intensities.
#pragma once
#include <math.h>
#include <stddef.h>

#if defined(__HIPCC__)
#define IA3_LAB_HD __host__ __device__
#else
#define IA3_LAB_HD
#endif

namespace ia3lab {

constexpr int MAX_RADIUS = 10;                                                    // spots_to_labels' own default
constexpr int MAX_CUBE = (2 * MAX_RADIUS + 1) * (2 * MAX_RADIUS + 1) * (2 * MAX_RADIUS + 1);   // 9261

// np.round(c).astype(np.int32): to the nearest integer, halves to the even one (2.5 -> 2, 3.5 -> 4, -0.5 -> 0).  A
// centre further than 2^30 from the origin is held there: with an offset of at most MAX_RADIUS it is clamped onto the
// same face of the image as the centre itself.  NaN is outside the contract.
IA3_LAB_HD inline int round_centre(double c) {
  const double lim = 1073741824.0;
  double r = rint(c);
  r = r < -lim ? -lim : (r > lim ? lim : r);
  return (int)r;
}

// an index that leaves [0, n) goes to the nearest face (partition_spots.py:230-232): clamped, not skipped
IA3_LAB_HD inline int clamp_index(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

// offset k of the cube of radius r: C order of (dz, dx, dy), dz slowest and dy fastest (:221-225)
IA3_LAB_HD inline void cube_offset(int k, int r, int* dz, int* dx, int* dy) {
  const int w = 2 * r + 1;
  const int q = k / w;
  *dy = k - q * w - r;
  const int p = q / w;
  *dx = q - p * w - r;
  *dz = p - r;
}

// flat index into a (Z, X, Y) stack of the voxel that offset k of the cube around the rounded centre (cz, cx, cy) reads
IA3_LAB_HD inline size_t cube_voxel(int cz, int cx, int cy, int k, int r, int Z, int X, int Y) {
  int dz, dx, dy;
  cube_offset(k, r, &dz, &dx, &dy);
  const int z = clamp_index(cz + dz, Z), x = clamp_index(cx + dx, X), y = clamp_index(cy + dy, Y);
  return ((size_t)z * X + x) * Y + y;
}

}  // namespace ia3lab
