// TEST INFRASTRUCTURE — host build of the index arithmetic of the label lookups (csrc/ia3_labels.h), the header labels.hip
// compiles for the device: centre rounding, offset order and clamping can be compared with NumPy on the CPU.  Not
// shipped, not a fallback.
#include "../../imageanalysis3_amd/csrc/ia3_labels.h"

extern "C" int ia3cpu_round_centre(double c) { return ia3lab::round_centre(c); }

// offsets: w^3 x 3 ints (dz, dx, dy) in the order the kernels walk the cube of radius r
extern "C" void ia3cpu_cube_offsets(int r, int* offsets) {
  const int w = 2 * r + 1;
  for (int k = 0; k < w * w * w; ++k) ia3lab::cube_offset(k, r, offsets + 3 * k, offsets + 3 * k + 1, offsets + 3 * k + 2);
}

// flat: n x w^3 flat voxel indices of the cubes around n centres (n x 3 float64) in a (Z, X, Y) stack
extern "C" void ia3cpu_cube_voxels(const double* centres, int n, int r, int Z, int X, int Y, long long* flat) {
  const int w = 2 * r + 1, w3 = w * w * w;
  for (int i = 0; i < n; ++i) {
    const int cz = ia3lab::round_centre(centres[3 * i]), cx = ia3lab::round_centre(centres[3 * i + 1]),
              cy = ia3lab::round_centre(centres[3 * i + 2]);
    for (int k = 0; k < w3; ++k) flat[(size_t)i * w3 + k] = (long long)ia3lab::cube_voxel(cz, cx, cy, k, r, Z, X, Y);
  }
}
