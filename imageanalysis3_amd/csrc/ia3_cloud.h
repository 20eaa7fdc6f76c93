// Host and device arithmetic of the density clouds (cloud.hip), free of any HIP include so that a host-only
// program can check it (tests/native/cloud_cpu.cpp).  visual_tools.py:68-72 gauss_ker and :87-110 add_source, once:
//   cl_size     s = int(max(sig) * size_fold), refused when it is not in 0 .. CL_S_MAX
//   cl_box      the box of a source against an image shape, all in integers
//   cl_disp     the fractional displacement -pos_int + pos
//   cl_term     u * u of one axis, u = ((coord - disp) - s / 2.) / (sig * sig), NumPy's operations in NumPy's order
//   cl_arg      the argument of exp from the three terms, in NumPy's order of the sum
//   cl_pair     which of (disp, sig) an axis of the kernel takes: np.swapaxes(np.indices(...), 0, 3) gives kernel index
//               [a, b, c] the coordinates (b, c, a), so axis 0 pairs with entry 2, axis 1 with entry 0, axis 2 with entry 1
// Translation units that include this are built without FMA contraction and without fast-math (the Makefile's EXACT).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define IA3_CL_HD __host__ __device__ inline
#else
#define IA3_CL_HD inline
#endif

namespace ia3cl {

constexpr int CL_T0 = 4, CL_T1 = 4, CL_T2 = 16;     // voxels of a tile along the three axes, one lane each
constexpr int CL_THREADS = CL_T0 * CL_T1 * CL_T2;   // 256
constexpr int CL_TERMS = CL_T0 + CL_T1 + CL_T2;     // table entries of one source in a tile
constexpr int CL_CHUNK = 64;                        // sources staged in LDS at a time: one per lane of a wave
constexpr int CL_S_MAX = 4096;                      // IA3_CLOUD_MAX_S
constexpr int CL_KER_S_MAX = 511;                   // IA3_CLOUD_MAX_KER_S: a bare kernel of at most 512**3 values
constexpr double CL_POS_MAX = 1073741824.0;         // 2**30: a source further out reaches no image
constexpr double CL_OUT = -1.0;                     // a table entry for a coordinate outside the box: u * u is never negative
constexpr double CL_CUT = -746.0;                   // exp(t) = +0 for t < CL_CUT in any correctly or faithfully rounded float64 exp

struct ClBox {
  int pmin[3];   // image index of kernel index 0 (pos_min, before the clamp)
  int lo[3];     // first image index written
  int hi[3];     // one past the last
};

IA3_CL_HD int cl_pair(int axis) { return axis == 0 ? 2 : axis - 1; }

// the truncation toward zero of np.array(x, dtype=int), for |x| < 2**31
IA3_CL_HD int cl_trunc(double x) { return (int)x; }

// visual_tools.py:93 int(max(sig) * size_fold).  0: *s is set; 1: a value that is not finite; 2: s outside 0 .. CL_S_MAX
IA3_CL_HD int cl_size(double s0, double s1, double s2, double size_fold, int* s) {
  if (!(s0 - s0 == 0.0) || !(s1 - s1 == 0.0) || !(s2 - s2 == 0.0) || !(size_fold - size_fold == 0.0)) return 1;
  double m = s0;
  if (s1 > m) m = s1;
  if (s2 > m) m = s2;
  const double v = m * size_fold;
  if (!(v > -1.0) || !(v < (double)CL_S_MAX + 1.0)) return 2;   // int() truncates: -0.5 is 0
  *s = (int)v;
  return 0;
}

// :98-102 in_im: an index at or past the shape becomes shape - 1 (so the last plane is never reached), one below 0 is 0
IA3_CL_HD int cl_in_im(long long p, int shape) { return p >= shape ? shape - 1 : (p < 0 ? 0 : (int)p); }

// :91-108.  pos_int = trunc(pos); pos_min = trunc(pos_int - (s + 1) / 2.): for an even s + 1 that is pos_int - (s + 1) / 2,
// for an odd one the half-integer pos_int - s / 2 - 0.5 goes toward zero, down when it is positive and up when negative.
// false: the box holds no voxel (also for a source further than CL_POS_MAX away, whose box cannot reach an image)
IA3_CL_HD bool cl_box(const double* pos, int s, const int* shape, ClBox* b) {
  bool any = true;
  for (int k = 0; k < 3; ++k) {
    if (!(pos[k] > -CL_POS_MAX && pos[k] < CL_POS_MAX) || shape[k] < 1) { b->pmin[k] = b->lo[k] = b->hi[k] = 0; any = false; continue; }
    const long long pi = cl_trunc(pos[k]);
    const long long n = (long long)s + 1;
    long long pmin;
    if ((n & 1) == 0) pmin = pi - n / 2;
    else { const long long w = pi - n / 2; pmin = w >= 1 ? w - 1 : w; }   // w - 0.5 toward zero
    const long long pmax = pmin + n;
    b->pmin[k] = (int)pmin;
    b->lo[k] = cl_in_im(pmin, shape[k]);
    b->hi[k] = cl_in_im(pmax, shape[k]);
    if (b->hi[k] <= b->lo[k]) any = false;
  }
  return any;
}

// :92 xyz_disp = -pos_int + pos: the sign changes in integers, so pos = -0.0 gives 0 + -0.0 = +0.0
IA3_CL_HD double cl_disp(double pos) { return (double)(-cl_trunc(pos)) + pos; }

// :72 ((xyz - disp - sxyz / 2.) / sig**2)**2 of one coordinate: the integer coordinate becomes float64 in the first
// subtraction, sig**2 is sig * sig and the outer power u * u
IA3_CL_HD double cl_term(long long coord, double disp, int s, double sig) {
  const double u = (((double)coord - disp) - (double)s / 2.) / (sig * sig);
  return u * u;
}

IA3_CL_HD bool cl_out(double term) { return term == CL_OUT; }

// :72 -np.sum(..., axis=3) / 2.: the three terms of a row are added left to right, kernel coordinate 0 first; t0, t1, t2 are
// the terms of the kernel's axes 0, 1, 2, which carry the coordinates 2, 0, 1
IA3_CL_HD double cl_arg(double t0, double t1, double t2) { return -((t1 + t2) + t0) / 2.; }

}  // namespace ia3cl
