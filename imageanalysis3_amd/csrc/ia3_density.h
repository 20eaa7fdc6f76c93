// Host and device arithmetic of the compartment densities (density.hip), free of any HIP include so that a
// host-only program can check it (tests/native/density_cpu.cpp):
//   dn_arg      the argument of exp for one (contributor, query) pair, NumPy's operations in NumPy's order
//   dn_weight   how often a contributor counts for a query under one key (A or B)
//   dn_pack     the staged word of a contributor: its copy and its two multiplicities
// Translation units that include this are built without FMA contraction and without fast-math (the Makefile's EXACT).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define IA3_DN_HD __host__ __device__ inline
#else
#define IA3_DN_HD inline
#endif

namespace ia3dn {

constexpr int DN_QTILE = 128;        // queries of a workgroup, one per lane
constexpr int DN_CTILE = 256;        // contributors staged in LDS at a time
constexpr int DN_PART = 64;          // contributors of one partial sum (the error bound of DESIGN.md §25 is stated for 64)
constexpr int DN_CELL_MAX = 65536;   // IA3_DENSITY_MAX_CELL: a copy number fits 16 bits
constexpr double DN_CUT = -746.0;    // exp(t) = +0 for t < DN_CUT in any correctly or faithfully rounded float64 exp
enum { DN_USE_CIS = 1, DN_USE_TRANS = 2, DN_EXCLUDE_SELF = 4 };

// density.py:7  -0.5 * np.sum((centers - ref_center)**2 / sigma**2, axis=-1): the power is x * x, the sum of three runs
// left to right, and the sign of d does not reach the square
IA3_DN_HD double dn_arg(double cz, double cx, double cy, double qz, double qx, double qy, double s2z, double s2x, double s2y) {
  const double dz = cz - qz, dx = cx - qx, dy = cy - qy;
  return -0.5 * ((dz * dz / s2z + dx * dx / s2x) + dy * dy / s2y);
}

// density.py:40-58: a contributor of another copy is listed `mult` times (the reference indexes with the list); one of the
// query's own copy once if it is listed at all (np.intersect1d), and never the query itself under exclude_self
IA3_DN_HD int dn_weight(bool same_copy, bool self, int mult, int flags) {
  if (!same_copy) return (flags & DN_USE_TRANS) ? mult : 0;
  if (!(flags & DN_USE_CIS) || mult == 0) return 0;
  return (self && (flags & DN_EXCLUDE_SELF)) ? 0 : 1;
}

IA3_DN_HD uint32_t dn_pack(int copy, int mult_a, int mult_b) {
  return (uint32_t)copy | ((uint32_t)mult_a << 16) | ((uint32_t)mult_b << 24);
}
IA3_DN_HD int dn_copy(uint32_t w) { return (int)(w & 0xffffu); }
IA3_DN_HD int dn_mult_a(uint32_t w) { return (int)((w >> 16) & 0xffu); }
IA3_DN_HD int dn_mult_b(uint32_t w) { return (int)(w >> 24); }

}  // namespace ia3dn
