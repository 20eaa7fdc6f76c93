// SciPy's cubic B-spline arithmetic (scipy.ndimage.map_coordinates, order 3), stated once for every kernel that has to
// reproduce it bit for bit: the prefilter of a line, the four tap weights, the 64-tap sum, the output cast and the
// order in which a warp composes its coordinate.  warp.hip (the warp of a stack) and calib.hip (the boxes of the
// chromatic-profile generator) are built from these pieces; a fix to a boundary sum or a rounding goes here and nowhere
// else.  Every line is part of the contract with SciPy: compile with -ffp-contract=off.
#pragma once
#include <math.h>
#include <stdint.h>

#include "warp_iir0_kernel.inc"   // NPAD, clampi, IirInit (the text the run-time compiler also builds: kept self-contained)

namespace ia3spline {
using namespace ia3warpk;

#define IA3_POLE3 (-0.26794919243112270647)   // sqrt(3) - 2, correctly rounded

// outputs: float32: cast; uint16: floor(t + 0.5) clamped to [0, 65535]
template <class T> __device__ __forceinline__ T out_cvt(double t);
template <> __device__ __forceinline__ float out_cvt<float>(double t) { return (float)t; }
template <> __device__ __forceinline__ uint16_t out_cvt<uint16_t>(double t) {
  t = t > 0 ? t + 0.5 : 0.0;
  t = t > 65535.0 ? 65535.0 : t;
  return (uint16_t)(int)t;
}

// x / 6.0, correctly rounded, without the division sequence (15-20 dependent instructions, nine of them per voxel in
// the cubic weights): q = RN(x * RN(1/6)) is within an ulp of the quotient, the remainder r = x - 6q is exact in one
// fused multiply-add, and RN(q + r * RN(1/6)) is then the correctly rounded quotient (Markstein's theorem; the weights
// are far from the overflow / underflow ranges where it needs help).
__device__ __forceinline__ double div6(double x) {
  const double y = 0x1.5555555555555p-3;
  const double q = x * y;
  const double r = __builtin_fma(-6.0, q, x);
  return __builtin_fma(r, y, q);
}

// the four tap weights of a coordinate with fraction yv = c - floor(c): w1 = (y²(y-2)·3+4)/6, w2 = (z²(z-2)·3+4)/6,
// w0 = z³/6, w3 = 1-w0-w1-w2 with z = 1-y, evaluated in SciPy's order
__device__ __forceinline__ void cubic_weights(double yv, double* w) {
  const double zv = 1.0 - yv;
  w[1] = div6(yv * yv * (yv - 2.0) * 3.0 + 4.0);
  w[2] = div6(zv * zv * (zv - 2.0) * 3.0 + 4.0);
  w[0] = div6(zv * zv * zv);
  w[3] = 1.0 - w[0] - w[1] - w[2];
}

// Two of the pieces below are macros, not functions.  An inlined function is simplified on its own before it reaches the
// kernel, and that fixes one form (selects or branches, loads hoisted or not) for every caller; the two gathers of
// warp.hip compile these lines differently, and warp_cubic4_k, which lives four registers under its occupancy limit, spills
// with every function-shaped variant that was tried.  The text of a macro is compiled where it stands, as it was.

// first of the four taps of a coordinate with floor fl on an axis of n samples, before the index clamp.  Far-away
// coordinates must not overflow int: every index beyond the range clamps to the same edge.
#define IA3_CUBIC_FIRST_TAP(fl, n) ((int)((fl) < -8.0 ? -8.0 : ((fl) > (double)(n) + 8.0 ? (double)(n) + 8.0 : (fl))) - 1)

// The coordinate a warp samples at: grid position, drift and (where there is one) the displacement field, composed in the
// order the caller of the reference composes them (fdt & 16):
//   set    (grid - drift) + field   classes/preprocess.py:923-935
//   clear  (grid + field) - drift   translate.py:19-25, io_tools/load.py:443-448
// warp_coord does it for the three axes of one output (cc: the grid position on entry; fld(a): component a of the field at
// this voxel, asked for only where there is a field); IA3_WARP_COORD is the same for one axis, for warp_cubic4_k, which
// holds the field values of its outputs in registers (a macro: see above).
#define IA3_WARP_COORD(c, drift, field, fdt, f)                    \
  do {                                                             \
    if ((fdt) & 16) { c = c - (drift); if (field) c = c + (f); }   \
    else { if (field) c = c + (f); c = c - (drift); }              \
  } while (0)
template <class F>
__device__ __forceinline__ void warp_coord(double* cc, const double* drift, const void* field, int fdt, F fld) {
  if (fdt & 16) {
    cc[0] = cc[0] - drift[0]; cc[1] = cc[1] - drift[1]; cc[2] = cc[2] - drift[2];
    if (field) { cc[0] = cc[0] + fld(0); cc[1] = cc[1] + fld(1); cc[2] = cc[2] + fld(2); }
  } else {
    if (field) { cc[0] = cc[0] + fld(0); cc[1] = cc[1] + fld(1); cc[2] = cc[2] + fld(2); }
    cc[0] = cc[0] - drift[0]; cc[1] = cc[1] - drift[1]; cc[2] = cc[2] - drift[2];
  }
}

// the 4 x 4 x 4 weighted sum in C order, every product as ((c*w0)*w1)*w2, over plain loads.  row(i0, i1): pointer to
// the coefficient row of indices i0, i1 along the first two axes; idx / w: [axis][tap]
template <class Row>
__device__ __forceinline__ double gather64(Row row, const int (*idx)[4], const double (*w)[4]) {
  double t = 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double* r = row(idx[0][i], idx[1][j]);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        double c = r[idx[2][k]];
        c = c * w[0][i]; c = c * w[1][j]; c = c * w[2][k];
        t = t + c;
      }
    }
  return t;
}

// the double whose low and high words a buffer load returned
__device__ __forceinline__ double words2double(unsigned lo, unsigned hi) { return __hiloint2double((int)hi, (int)lo); }

// ---- prefilter of a line ('nearest' / 'reflect' boundary: half-sample-symmetric) -----------------------------------------
// host: what the recursions of a line of n samples need (IirInit): gain (1-z)(1-1/z), zn = z^n by the host's pow,
// scale = z / (1 - zn²); full where z^n has not underflowed.  bound / amax_bits (the cut of long lines) are the caller's.
inline IirInit iir_init(int n) {
  IirInit q;
  q.z = IA3_POLE3;
  q.gain = (1.0 - q.z) * (1.0 - 1.0 / q.z);
  q.zn = pow(q.z, (double)n);
  q.scale = q.z / (1.0 - q.zn * q.zn);
  q.full = q.zn != 0.0 ? 1 : 0;
  q.bound = 0.0;
  q.amax_bits = nullptr;
  return q;
}

// start-of-line value of the causal recursion
// The sum runs over the whole line in SciPy.  When z^n underflows to zero (n >= 566) the mirror terms vanish exactly and
// the sum is cut where the rest provably cannot change it: every remaining term is at most |z|^i * bound in magnitude
// (bound = gain * largest |sample| the pass can meet), and an addend below a quarter ulp of the running sum leaves it
// unchanged under round-to-nearest, so once |sum| * 2^-55 > |z|^i * bound all further additions are no-ops.  The test
// is made after 64 terms and every 64 terms from there; a line whose leading samples are zero simply reads on.  The
// largest sample is 65535 for uint16 sources and is measured for float32 ones (warp.hip: absmax_f32_k); each pass of the
// prefilter can raise it by at most a factor 3 (the absolute sum of its impulse response).

__device__ __forceinline__ double iir_bound(const IirInit& q) {
  return q.amax_bits ? q.bound * (double)__uint_as_float(*q.amax_bits) : q.bound;
}
// true when no later term of the start sum can change `s` (see IirInit); NaN / inf bounds never pass
__device__ __forceinline__ bool iir_sum_settled(double s, double zi, double bound) {
  return fabs(s) * 0x1p-55 > fabs(zi) * bound || (zi == 0.0 && bound < INFINITY);
}

// start value of the causal recursion of a strided line (element i at c + i*stride), see IirInit
__device__ __forceinline__ double iir_start_strided(const double* __restrict__ c, size_t stride, int n, const IirInit& q) {
  const double z = q.z, g = q.gain;
  const double c0 = c[0] * g;
  double s;
  if (q.full) {
    s = c0 + q.zn * (c[(size_t)(n - 1) * stride] * g);
    double zi = z;
    for (int i = 1; i < n; ++i) {
      s += zi * (c[(size_t)i * stride] * g + q.zn * (c[(size_t)(n - 1 - i) * stride] * g));
      zi *= z;
    }
  } else {
    const double bound = iir_bound(q);
    s = c0;
    double zi = z;
    for (int i = 1; i < n;) {
      const int e = i + 63 < n ? i + 63 : n;
      for (; i < e; ++i) { s += zi * (c[(size_t)i * stride] * g); zi *= z; }
      if (iir_sum_settled(s, zi, bound)) break;
    }
  }
  s *= q.scale;
  s += c0;
  return s;
}

// Two sweeps over a strided line, in place, from sample `from` (whose causal value `first` is known) to the end and
// back: [from, n) holds raw samples on entry and coefficients on exit.
// The recursions are serial in `prev`, their loads are not: eight samples are fetched ahead of the eight dependent
// updates, so a thread keeps eight loads in flight instead of one (the kernel ran at 1.6 TB/s, latency-bound).
// MIRROR: the anticausal start of the whole-sample-symmetric boundary (mode 'constant', warp.hip) instead of the
// half-sample-symmetric one; needs the causal values of the last TWO samples (from <= n - 2).
template <bool MIRROR = false>
__device__ __forceinline__ void iir_two_sweeps_strided(double* __restrict__ c, size_t stride, int from, int n, double first,
                                                       double z, double g) {
  constexpr int B = 8;   // 16 in flight: no faster (2.36 against 2.25 ms)
  double prev = first;
  c[(size_t)from * stride] = prev;
  int i = from + 1;
  for (; i + B <= n; i += B) {
    double in[B];
#pragma unroll
    for (int k = 0; k < B; ++k) in[k] = c[(size_t)(i + k) * stride];
#pragma unroll
    for (int k = 0; k < B; ++k) {
      const double v = in[k] * g + z * prev;
      c[(size_t)(i + k) * stride] = v;
      prev = v;
    }
  }
  for (; i < n; ++i) {
    double v = c[(size_t)i * stride] * g + z * prev;
    c[(size_t)i * stride] = v;
    prev = v;
  }
  if (MIRROR) prev = ((z * c[(size_t)(n - 2) * stride] + prev) * z) / (z * z - 1.0);   // (c[n-2]: this thread's own store)
  else prev = prev * (z / (z - 1.0));
  c[(size_t)(n - 1) * stride] = prev;
  i = n - 2;
  for (; i - (B - 1) >= from; i -= B) {
    double in[B];
#pragma unroll
    for (int k = 0; k < B; ++k) in[k] = c[(size_t)(i - k) * stride];
#pragma unroll
    for (int k = 0; k < B; ++k) {
      const double v = z * (prev - in[k]);
      c[(size_t)(i - k) * stride] = v;
      prev = v;
    }
  }
  for (; i >= from; --i) {
    double v = z * (prev - c[(size_t)i * stride]);
    c[(size_t)i * stride] = v;
    prev = v;
  }
}

}  // namespace ia3spline
