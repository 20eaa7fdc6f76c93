// The certificate behind the plane skipping of seed_front_k (seed.hip): an upper bound of max_im over a unit (tile, plane)
// from the largest value of the kernel's INPUT (the short filter's axis-0 result) over the unit's in-plane window.
// Compiles for host and device; tests/native/seedskip_cpu.cpp exposes it to the CPU suite.
//
// max_im(x, y) on a plane is two 7-tap passes over that plane of the input, each
//     acc = v[3] * w0;  acc = acc + (v[3-j] + v[3+j]) * wj  (j = 3, 2, 1; f64, round to nearest, unfused);  out = cvt<T>(acc)
// over rows x-3 .. x+3 and columns y-3 .. y+3 with 'reflect' indices, which stay inside the window clamped to the image.
//
// Claim: with every tap >= 0, m >= 0 the largest input value in the window (NaN left out), S the taps' sum,
// SUP = S * (1 + 2^-40) and q = cvt<T> on [0, top of T's range):   max_im <= U(m) = q(fl(q(fl(m * SUP)) * SUP)).
//  * Every operation of a pass (product with a non-negative tap, sum, rounding) is non-decreasing in its operands, so the
//    computed acc is at or below the acc of the constant window m.  For that one the four roundings on the longest chain
//    give acc <= m * S_exact * (1 + 2^-53)^4 (+ 2^-1073 where a product underflows; v + v is exact).  S as summed on the
//    host is within (1 + 2^-53)^4 of S_exact, and fl(m * SUP) >= m * SUP * (1 - 2^-53), so fl(m * SUP) covers it with
//    2^-40 against 9 * 2^-53 (the absolute term too: S is required to lie in [2^-64, 2^64], and a non-zero m is at least
//    2^-149, so m * S >= 2^-213).  m = 0 gives 0.
//  * cvt<T> is non-decreasing where it does not wrap: float32 rounds to nearest (an overflow is +inf: live); uint16
//    truncates, and a bound at or above 65536 makes no claim (the unit is live).  So the axis-1 result is at or below
//    a = q(fl(m * SUP)) everywhere in the window, and the same step again bounds the axis-2 result.
//  * A negative maximum (or none: every value NaN) makes no claim either: U = +inf, the unit is live.
//  * NaN: a max_im that is NaN is never a candidate (vmax == cmax fails), and a finite max_im has 49 finite inputs, all
//    at or below m because NaN is left out of m.  +inf in the window gives m = +inf: live.  (The column kernel's integer
//    reduction leaves out a NaN whose sign bit is set and reports NaN for a strip that holds one with the bit clear;
//    seed_front_k reads a NaN strip as +inf.  Both are at or above the maximum of the strip's other values.)
// A unit is live when U - bound >= th_test with the detector's own bound and threshold: the detector's test is
// (double)cmax - bound >= th_test with cmax <= U, and the f64 subtraction is non-decreasing in cmax.  (bound = NaN or
// +inf fails both tests; bound = -inf passes both.)
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define IA3_SKIP_HD __host__ __device__ inline
#else
#define IA3_SKIP_HD inline
#endif

namespace ia3skip {

// taps w[0..3] (centre first) of the radius-3 front filter -> SUP; false (no skipping) when a tap is negative or NaN or the
// sum is outside [2^-64, 2^64]
IA3_SKIP_HD bool taps_sup(const double* w, double* sup) {
  for (int j = 0; j < 4; ++j)
    if (!(w[j] >= 0.0)) return false;
  const double s = w[0] + 2.0 * (w[1] + w[2] + w[3]);
  if (!(s >= 5.421010862427522e-20 && s <= 18446744073709551616.0)) return false;
  *sup = s * (1.0 + 9.094947017729282e-13);   // 2^-40
  return true;
}

template <bool U16> IA3_SKIP_HD double pass_bound(double m, double sup) {   // m >= 0 or +inf
  const double v = m * sup;
  if (U16) return v < 65536.0 ? (double)(uint16_t)(int)v : INFINITY;
  return (double)(float)v;
}

// certified upper bound of max_im over a unit whose window maximum is m
template <bool U16> IA3_SKIP_HD double front_bound(float m, double sup) {
  if (!(m >= 0.f)) return INFINITY;
  const double a = pass_bound<U16>((double)m, sup);
  return a < INFINITY ? pass_bound<U16>(a, sup) : INFINITY;
}

// the unit can hold a first-stage candidate
IA3_SKIP_HD bool unit_live(double ubound, double bound, double th_test) { return ubound - bound >= th_test; }

}  // namespace ia3skip
