// Order statistics of a resident stack and the illumination-profile reduction built on them (reference:
// correction_tools/illumination.py:146-194 _image_to_profile):
//   scoreatpercentile(im, per)   exact: radix select of the order-preserving key, up to 16 ranks per set of passes
//   sum_z clip(float64(im))      one thread per (x, y) column, planes added in z order
//   gaussian_filter(f64 (X, Y))  NI_Correlate1D's summation order, axis 0 then axis 1
// Everything is integer selection or float64 arithmetic in a fixed order, so results equal NumPy / SciPy bit for bit.
//
// The select is ia3_select.h's, asked for one segment: the whole stack.
#include "ia3_rt.h"
#include "ia3_select.h"
#include "ia3_gauss_dev.h"
#include <math.h>
#include <vector>

using namespace ia3rt;

namespace {

constexpr int GAUSS_MAX_RADIUS = 1024;

// ---- sum over z of the (clamped) float64 voxels -----------------------------------------------------------------
template <class T> struct VecOf;
template <> struct VecOf<uint16_t> { typedef uint2 type; };   // 4 x uint16
template <> struct VecOf<float> { typedef uint4 type; };      // 4 x float32

__device__ __forceinline__ double clampd(double v, double lo, double hi) {   // np.clip: NaN stays NaN
  return v < lo ? lo : (v > hi ? hi : v);
}

// V adjacent columns per thread (V = 4 needs plane % 4 == 0 and an aligned base, else V = 1); acc = plane 0, then
// acc = acc + plane z for z = 1 .. Z-1: np.sum(axis=0) of a float64 (Z, X, Y) array
template <class T, int V>
__global__ __launch_bounds__(256) void clip_sum_z_k(const T* __restrict__ im, int Z, size_t plane, int clip, double lo,
                                                    double hi, double* __restrict__ out) {
  const size_t c = ((size_t)blockIdx.x * 256 + threadIdx.x) * V;
  if (c >= plane) return;
  double acc[V];
  for (int z = 0; z < Z; ++z) {
    T e[V];
    if constexpr (V == 1) e[0] = im[(size_t)z * plane + c];
    else {
      const typename VecOf<T>::type q = *(const typename VecOf<T>::type*)(im + (size_t)z * plane + c);
      __builtin_memcpy(e, &q, sizeof(q));
    }
#pragma unroll
    for (int j = 0; j < V; ++j) {
      double v = (double)e[j];
      if (clip) v = clampd(v, lo, hi);
      acc[j] = z == 0 ? v : acc[j] + v;
    }
  }
#pragma unroll
  for (int j = 0; j < V; ++j) out[c + j] = acc[j];
}

// ---- float64 correlation along one axis of a 2-D image ------------------------------------------------------------
// A block makes T consecutive outputs of C neighbouring lines from an LDS tile of T + 2R positions (border indices
// resolved while it is filled).  Element (line l, position t) lives at l * ls + t * ts: the pass along the rows' axis
// (axis 0, ts = Y) takes C = 2 adjacent columns so that LDS reads of a wave stay consecutive; the pass along the
// contiguous axis takes C = 1.  Per output NI_Correlate1D's symmetric sequence, no contraction:
//   acc = in[0] * w[R];  for j = R .. 1: acc += (in[-j] + in[+j]) * w[R - j]
template <int C>
__global__ __launch_bounds__(256) void corr1d_f64_k(const double* __restrict__ in, int lines, int len, size_t ls, size_t ts,
                                                    const double* __restrict__ w, int R, int mode,
                                                    double* __restrict__ out) {
  extern __shared__ double s[];
  constexpr int T = 256 / C;
  const int t0 = blockIdx.x * T, l0 = blockIdx.y * C;
  const int span = T + 2 * R;
  for (int i = threadIdx.x; i < span * C; i += 256) {
    const int pos = i / C, c = i % C;
    const int l = l0 + c;
    double v = 0.0;
    if (l < lines) v = in[(size_t)l * ls + (size_t)ia3g::border_idx(t0 + pos - R, len, mode) * ts];
    s[i] = v;
  }
  __syncthreads();
  const int c = threadIdx.x % C, tl = threadIdx.x / C;
  const int l = l0 + c, t = t0 + tl;
  if (l >= lines || t >= len) return;
  const double* p = s + (size_t)(tl + R) * C + c;
  double acc = p[0] * w[R];
  for (int j = R; j >= 1; --j) acc += (p[-j * C] + p[j * C]) * w[R - j];
  out[(size_t)l * ls + (size_t)t * ts] = acc;
}

int check_stack(const ia3_stack* s) {
  if (!s || !s->d) return set_error(IA3_EINVAL, "null stack");
  if (s->dtype != IA3_U16 && s->dtype != IA3_F32) return set_error(IA3_EINVAL, "stack dtype must be uint16 or float32");
  if (s->Z < 1 || s->X < 1 || s->Y < 1) return set_error(IA3_EINVAL, "empty stack");
  return IA3_OK;
}

// the n order statistics, left in `dout` (n values of the stack dtype, device)
int order_stats(const ia3_stack* s, const long long* ranks, int n, void* dout) {
  const size_t nvox = (size_t)s->Z * s->X * s->Y;
  SelRanks r{};
  for (int i = 0; i < n; ++i) r.k[i] = (u64)ranks[i];
  r.n = n;
  Select<false> sel(1);
  if (!sel.ok()) return IA3_ENOMEM;
  ProfScope ps("order_stats");
  if (s->dtype == IA3_F32) {
    int rc = sel.run((const float*)s->d, nvox, r); if (rc) return rc;
    return sel.values((float*)dout);
  }
  int rc = sel.run((const uint16_t*)s->d, nvox, r); if (rc) return rc;
  return sel.values((uint16_t*)dout);
}

int check_ranks(const ia3_stack* s, const long long* ranks, int n) {
  if (!ranks || n < 1) return set_error(IA3_EINVAL, "at least one rank is required");
  if (n > MAXR) return set_error(IA3_EINVAL, "at most %d ranks per call, got %d", MAXR, n);
  const long long nvox = (long long)s->Z * s->X * s->Y;
  for (int i = 0; i < n; ++i)
    if (ranks[i] < 0 || ranks[i] >= nvox) return set_error(IA3_EINVAL, "rank %lld outside [0, %lld)", ranks[i], nvox);
  return IA3_OK;
}

int order_stats_host(const ia3_stack* s, const long long* ranks, int n, void* out) {
  Scratch dout(MAXR * sizeof(float));
  if (!dout.p) return IA3_ENOMEM;
  int rc = order_stats(s, ranks, n, dout.p); if (rc) return rc;
  return fetch(dout.as<char>(), (size_t)n * esize(s->dtype), (char*)out);
}

int clip_sum_z(const ia3_stack* s, int clip, double lo, double hi, double* out_dev) {
  hipStream_t st = stream();
  const size_t plane = (size_t)s->X * s->Y;
  const bool f32 = s->dtype == IA3_F32;
  const bool vec = plane % 4 == 0 && ((uintptr_t)s->d & 15) == 0;
  const size_t threads = vec ? plane / 4 : plane;
  const unsigned gx = (unsigned)((threads + 255) / 256);
  ProfScope ps("clip_sum_z");
  if (f32) {
    if (vec) hipLaunchKernelGGL((clip_sum_z_k<float, 4>), dim3(gx), dim3(256), 0, st, (const float*)s->d, s->Z, plane, clip, lo, hi, out_dev);
    else hipLaunchKernelGGL((clip_sum_z_k<float, 1>), dim3(gx), dim3(256), 0, st, (const float*)s->d, s->Z, plane, clip, lo, hi, out_dev);
  } else {
    if (vec) hipLaunchKernelGGL((clip_sum_z_k<uint16_t, 4>), dim3(gx), dim3(256), 0, st, (const uint16_t*)s->d, s->Z, plane, clip, lo, hi, out_dev);
    else hipLaunchKernelGGL((clip_sum_z_k<uint16_t, 1>), dim3(gx), dim3(256), 0, st, (const uint16_t*)s->d, s->Z, plane, clip, lo, hi, out_dev);
  }
  IA3_KCHECK();
  return IA3_OK;
}

// scipy.ndimage.gaussian_filter of a float64 (X, Y) image: in_dev -> out_dev (may be the same buffer).  weights: the
// 2 * radius + 1 taps SciPy would use, from NumPy on the caller's side (bit-equal results need NumPy's own exp, which
// differs from libm's in the last bit for some arguments); NULL: made here from (sigma, truncate).
int gaussian2d_f64(const double* in_dev, int X, int Y, double sigma, double truncate, int mode, const double* weights,
                   int radius, double* out_dev) {
  if (X < 1 || Y < 1) return set_error(IA3_EINVAL, "empty image");
  if (mode != IA3_MODE_REFLECT && mode != IA3_MODE_NEAREST)
    return set_error(IA3_EUNSUPPORTED, "the float64 Gaussian takes mode reflect or nearest");
  if (X > 32768 || Y > 32768) return set_error(IA3_EUNSUPPORTED, "images of up to 32768 x 32768 are supported");
  std::vector<double> w; int R;
  if (weights) {
    if (radius < 0) return set_error(IA3_EINVAL, "negative filter radius");
    if (radius > GAUSS_MAX_RADIUS) return set_error(IA3_EUNSUPPORTED, "filter radius %d above the supported %d", radius, GAUSS_MAX_RADIUS);
    R = radius;
    w.assign(weights, weights + 2 * (size_t)R + 1);
  } else {
    if (!(sigma > 0) || !(truncate > 0)) return set_error(IA3_EINVAL, "sigma and truncate must be positive");
    if (truncate * sigma + 0.5 >= (double)GAUSS_MAX_RADIUS + 1.0)   // radius = int(truncate * sigma + 0.5), before any tap is made
      return set_error(IA3_EUNSUPPORTED, "filter radius %.0f above the supported %d", floor(truncate * sigma + 0.5), GAUSS_MAX_RADIUS);
    gaussian_taps(sigma, truncate, w, R);
  }
  hipStream_t st = stream();
  const size_t bytes = (size_t)X * Y * sizeof(double);
  Scratch dw(w.size() * sizeof(double)), tmp(bytes);
  if (!dw.p || !tmp.p) return IA3_ENOMEM;
  IA3_HIP(hipMemcpyAsync(dw.p, w.data(), w.size() * sizeof(double), hipMemcpyHostToDevice, st));   // pageable: staged on return
  ProfScope ps("gaussian2d_f64");
  {   // axis 0: lines = columns y (stride 1), positions along x (stride Y)
    constexpr int C = 2, T = 256 / C;
    const size_t lds = (size_t)(T + 2 * R) * C * sizeof(double);
    hipLaunchKernelGGL((corr1d_f64_k<C>), dim3((X + T - 1) / T, (Y + C - 1) / C), dim3(256), lds, st, in_dev, Y, X, (size_t)1,
                       (size_t)Y, (const double*)dw.p, R, mode, tmp.as<double>());
  }
  {   // axis 1: lines = rows x (stride Y), positions along y (stride 1)
    constexpr int T = 256;
    const size_t lds = (size_t)(T + 2 * R) * sizeof(double);
    hipLaunchKernelGGL((corr1d_f64_k<1>), dim3((Y + T - 1) / T, X), dim3(256), lds, st, (const double*)tmp.p, X, Y, (size_t)Y,
                       (size_t)1, (const double*)dw.p, R, mode, out_dev);
  }
  IA3_KCHECK();
  return IA3_OK;
}

}  // namespace

extern "C" {

int ia3_stack_order_stats_dev(const ia3_stack* s, const long long* ranks, int n, void* out) {
  int rc = ensure_init(); if (rc) return rc;
  rc = check_stack(s); if (rc) return rc;
  rc = check_ranks(s, ranks, n); if (rc) return rc;
  if (!out) return set_error(IA3_EINVAL, "null output");
  return order_stats_host(s, ranks, n, out);
}

int ia3_stack_percentiles_dev(const ia3_stack* s, const double* pers, int n, double* out) {
  int rc = ensure_init(); if (rc) return rc;
  rc = check_stack(s); if (rc) return rc;
  if (!pers || !out || n < 1) return set_error(IA3_EINVAL, "at least one percentile is required");
  if (2 * n > MAXR) return set_error(IA3_EINVAL, "at most %d percentiles per call, got %d", MAXR / 2, n);
  const long long nvox = (long long)s->Z * s->X * s->Y;
  long long ranks[MAXR], lo[MAXR];
  double idx[MAXR];
  for (int i = 0; i < n; ++i) {
    if (!(pers[i] >= 0 && pers[i] <= 100)) return set_error(IA3_EINVAL, "percentile must be in the range [0, 100]");
    percentile_index(pers[i], nvox, &lo[i], &idx[i]);
    ranks[2 * i] = lo[i];
    ranks[2 * i + 1] = percentile_next(lo[i], nvox);
  }
  union { uint16_t u[MAXR]; float f[MAXR]; } v;
  rc = order_stats_host(s, ranks, 2 * n, &v); if (rc) return rc;
  for (int i = 0; i < n; ++i) {
    const double s0 = s->dtype == IA3_F32 ? (double)v.f[2 * i] : (double)v.u[2 * i];
    const double s1 = s->dtype == IA3_F32 ? (double)v.f[2 * i + 1] : (double)v.u[2 * i + 1];
    out[i] = percentile_value(idx[i], lo[i], s0, s1);
  }
  return IA3_OK;
}

int ia3_clip_sum_z_dev(const ia3_stack* s, int clip, double lo, double hi, double* out_dev) {
  int rc = ensure_init(); if (rc) return rc;
  rc = check_stack(s); if (rc) return rc;
  if (!out_dev) return set_error(IA3_EINVAL, "null output");
  if (clip && !(lo <= hi)) return set_error(IA3_EINVAL, "clip limits must be ordered, got [%g, %g]", lo, hi);
  return clip_sum_z(s, clip, lo, hi, out_dev);
}

int ia3_gaussian_filter2d_f64_dev(const double* in_dev, int X, int Y, double sigma, double truncate, int mode,
                                  const double* weights, int radius, double* out_dev) {
  int rc = ensure_init(); if (rc) return rc;
  if (!in_dev || !out_dev) return set_error(IA3_EINVAL, "null argument");
  return gaussian2d_f64(in_dev, X, Y, sigma, truncate, mode, weights, radius, out_dev);
}

int ia3_gaussian_filter2d_f64(const double* in, int X, int Y, double sigma, double truncate, int mode,
                              const double* weights, int radius, double* out) {
  int rc = ensure_init(); if (rc) return rc;
  if (!in || !out) return set_error(IA3_EINVAL, "null argument");
  if (X < 1 || Y < 1) return set_error(IA3_EINVAL, "empty image");
  const size_t bytes = (size_t)X * Y * sizeof(double);
  Scratch d(bytes);
  if (!d.p) return IA3_ENOMEM;
  hipStream_t st = stream();
  IA3_HIP(hipMemcpyAsync(d.p, in, bytes, hipMemcpyHostToDevice, st));
  rc = gaussian2d_f64(d.as<double>(), X, Y, sigma, truncate, mode, weights, radius, d.as<double>()); if (rc) return rc;
  IA3_HIP(hipMemcpyAsync(out, d.p, bytes, hipMemcpyDeviceToHost, st));
  IA3_HIP(hipStreamSynchronize(st));
  return IA3_OK;
}

// correction_tools/illumination.py:181-190 for one channel stack
int ia3_illumination_image_profile_dev(const ia3_stack* im, int remove_cap, double per_a, double per_b, double sigma,
                                       const double* weights, int radius, double* out_host) {
  int rc = ensure_init(); if (rc) return rc;
  rc = check_stack(im); if (rc) return rc;
  if (!out_host) return set_error(IA3_EINVAL, "null output");
  double lo = 0, hi = 0;
  if (remove_cap) {
    // the reference asks for min(cap_th_per) and max(cap_th_per) and orders the two limits once more
    const double pers[2] = {per_a < per_b ? per_a : per_b, per_a < per_b ? per_b : per_a};
    double lim[2];
    rc = ia3_stack_percentiles_dev(im, pers, 2, lim); if (rc) return rc;
    lo = lim[0] < lim[1] ? lim[0] : lim[1];
    hi = lim[0] < lim[1] ? lim[1] : lim[0];
  }
  const size_t bytes = (size_t)im->X * im->Y * sizeof(double);
  Scratch d(bytes);
  if (!d.p) return IA3_ENOMEM;
  rc = clip_sum_z(im, remove_cap ? 1 : 0, lo, hi, d.as<double>()); if (rc) return rc;
  rc = gaussian2d_f64(d.as<double>(), im->X, im->Y, sigma, 4.0, IA3_MODE_REFLECT, weights, radius, d.as<double>()); if (rc) return rc;
  IA3_HIP(hipMemcpyAsync(out_host, d.p, bytes, hipMemcpyDeviceToHost, stream()));
  IA3_HIP(hipStreamSynchronize(stream()));
  return IA3_OK;
}

}  // extern "C"
