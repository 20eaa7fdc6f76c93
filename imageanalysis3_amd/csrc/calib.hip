// Device side of the chromatic-aberration profile generator (reference: correction_tools/chromatic.py:119-412).
//
// crop_pairs_k   io_tools/crop.py:107-152 crop_neighboring_area for n pairs of centres on two resident stacks, one
//                workgroup per pair, followed by the regression of the second box on the first (chromatic.py:387-390:
//                sklearn LinearRegression().fit / .score) from exact integer sums.  Per stack and pair:
//                  a. rough crop  [max(0, floor(c - crop/2)), min(size, ceil(c + crop/2)))
//                  b. positions   idx + ((c - left) - (crop - 1)/2), float64, in this order
//                  c. map_coordinates(order=3, mode='nearest') of the rough crop: edge-padded by 12, cubic B-spline
//                     prefilter along axes 0, 1, 2 in float64 (ia3_spline.h: the start sum and the two sweeps of the warp; a
//                     padded line has at most 41 samples, z^n is far from underflow and the start sum is SciPy's full one),
//                     the position + 12 clamped to the padded array, 4 x 4 x 4 taps in C order with clamped indices
//                     (ia3_spline.h: weights and sum)
//                  d. uint16: floor(t + 0.5) clamped; float32: cast
//                The padded coefficient volume of a pair (at most 41^3 doubles) lives in a slab of the workspace cache.
// poly_field_k   the dense (3, Z, X, Y) polynomial displacement field of chromatic.py:282-289: per axis the sum, left to
//                right over the columns of generate_polynomial_data, of C[k] * monomial_k(z - r0, x - r1, y - r2) in
//                float64.  A pure store stream.
// bleed_profile_k  the tail of the bleedthrough generator (correction_tools/bleedthrough.py:451-486): per pixel the
//                C x C matrix of slope polynomials (diagonal 1), its mean over z (sequential sum divided by Z) and its
//                inverse by Gaussian elimination with partial pivoting, all in registers.  Reads nothing.
// Compiled with -ffp-contract=off.
#include "ia3_rt.h"
#include <math.h>

using namespace ia3rt;

#include "ia3_spline.h"
using namespace ia3spline;

namespace {

constexpr int CROP_MAX = 15;
constexpr int ROUGH_MAX = CROP_MAX + 2;           // ceil(c + crop/2) - floor(c - crop/2) <= crop + 1 (+ 1: rounding of the two sums)
constexpr int PADLEN_MAX = ROUGH_MAX + 2 * NPAD;    // 41
constexpr int PADLEN_MIN = 1 + 2 * NPAD;            // 25

// what the prefilter needs per padded line length n (index n - PADLEN_MIN), made on the host (iir_init): the start sum is
// the full one at these lengths, bound and amax_bits are not read
struct SplineTab {
  IirInit q[PADLEN_MAX - PADLEN_MIN + 1];
};

struct CropGeom {
  int left[3], n[3];   // rough crop [left, left + n)
  double t[3];         // position of output index 0 in the rough crop
};

// crop.py:133-144 for one centre; false: the rough crop is empty along an axis (the reference then fails inside SciPy)
__host__ __device__ inline bool crop_geometry(const double* c, const int* crop, const int* dims, CropGeom& g) {
  bool ok = true;
  for (int a = 0; a < 3; ++a) {
    const double h = (double)crop[a] / 2.0;
    double lo = floor(c[a] - h), hi = ceil(c[a] + h);
    lo = lo > 0.0 ? lo : 0.0;
    hi = hi < (double)dims[a] ? hi : (double)dims[a];
    ok = ok && hi - lo >= 1.0 && hi - lo <= (double)(crop[a] + 2);   // (NaN centres fail here; the slab holds crop + 2)
    g.left[a] = ok ? (int)lo : 0;
    g.n[a] = ok ? (int)hi - (int)lo : 1;
    g.t[a] = (c[a] - lo) - (double)(crop[a] - 1) / 2.0;
  }
  return ok;
}

// one box of one stack; every thread of the workgroup takes part.  P: this workgroup's slab (>= the padded rough crop)
template <class T>
__device__ void crop_box(const T* __restrict__ im, int Z, int X, int Y, const double* __restrict__ centre, const int* crop,
                         const SplineTab& tab, double* P, T* out) {
  const int dims[3] = {Z, X, Y};
  const double c[3] = {centre[0], centre[1], centre[2]};
  CropGeom g;
  crop_geometry(c, crop, dims, g);   // (checked on the host: never empty)
  const int n0 = g.n[0] + 2 * NPAD, n1 = g.n[1] + 2 * NPAD, n2 = g.n[2] + 2 * NPAD;
  const int plane = n1 * n2, vol = n0 * plane;
  const int tid = threadIdx.x;
  for (int i = tid; i < vol; i += 256) {
    const int z = i / plane, r = i - z * plane, x = r / n2, y = r - x * n2;
    const int sz = g.left[0] + clampi(z - NPAD, g.n[0]), sx = g.left[1] + clampi(x - NPAD, g.n[1]),
              sy = g.left[2] + clampi(y - NPAD, g.n[2]);
    P[i] = (double)im[((size_t)sz * X + sx) * Y + sy];
  }
  __syncthreads();
  // the cubic prefilter of one strided line in place
  auto spline_line = [&](double* c, int stride, int n) {
    const IirInit& q = tab.q[n - PADLEN_MIN];
    iir_two_sweeps_strided(c, (size_t)stride, 0, n, iir_start_strided(c, (size_t)stride, n, q), q.z, q.gain);
  };
  for (int p = tid; p < plane; p += 256) spline_line(P + p, plane, n0);
  __syncthreads();
  for (int p = tid; p < n0 * n2; p += 256) {
    const int z = p / n2, y = p - z * n2;
    spline_line(P + z * plane + y, n2, n1);
  }
  __syncthreads();
  for (int p = tid; p < n0 * n1; p += 256) spline_line(P + p * n2, 1, n2);
  __syncthreads();
  const int np[3] = {n0, n1, n2};
  const int cvol = crop[0] * crop[1] * crop[2];
  for (int o = tid; o < cvol; o += 256) {
    const int i0 = o / (crop[1] * crop[2]), r = o - i0 * crop[1] * crop[2], i1 = r / crop[2], i2 = r - i1 * crop[2];
    const int id[3] = {i0, i1, i2};
    int idx[3][4]; double w[3][4];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      double cc = (double)id[a] + g.t[a];
      cc = cc + (double)NPAD;
      cc = cc < 0.0 ? 0.0 : (cc > (double)(np[a] - 1) ? (double)(np[a] - 1) : cc);   // mode 'nearest' on the padded array
      const double fl = floor(cc);
      cubic_weights(cc - fl, w[a]);
      const int st = (int)fl - 1;
#pragma unroll
      for (int k = 0; k < 4; ++k) idx[a][k] = clampi(st + k, np[a]);
    }
    out[o] = out_cvt<T>(gather64([&](int i0, int i1) { return (const double*)P + i0 * plane + i1 * n2; }, idx, w));
  }
  __syncthreads();
}

// reg (optional, uint16 only): per pair [slope, intercept, r^2] of box b on box a
template <class T>
__global__ __launch_bounds__(256) void crop_pairs_k(const T* __restrict__ a, const T* __restrict__ b, int Z, int X, int Y,
                                                    const double* __restrict__ ca, const double* __restrict__ cb, int c0, int c1,
                                                    int c2, SplineTab tab, double* __restrict__ slabs, size_t slab,
                                                    T* __restrict__ out_a, T* __restrict__ out_b, double* __restrict__ reg) {
  const int pair = blockIdx.x;
  const int crop[3] = {c0, c1, c2};
  const int cvol = c0 * c1 * c2;
  double* P = slabs + (size_t)pair * slab;
  T* oa = out_a + (size_t)pair * cvol;
  crop_box<T>(a, Z, X, Y, ca + 3 * (size_t)pair, crop, tab, P, oa);
  if (!b) return;
  T* ob = out_b + (size_t)pair * cvol;
  crop_box<T>(b, Z, X, Y, cb + 3 * (size_t)pair, crop, tab, P, ob);
  if (!reg) return;
  if constexpr (sizeof(T) == 2) {
    // exact sums: 15^3 voxels of uint16 keep every one below 2^44, and n * sum below 2^56
    __shared__ unsigned long long red[5][256];
    unsigned long long sx = 0, sy = 0, sxx = 0, sxy = 0, syy = 0;
    for (int o = threadIdx.x; o < cvol; o += 256) {   // (written by this workgroup, behind crop_box's barrier)
      const unsigned long long x = oa[o], y = ob[o];
      sx += x; sy += y; sxx += x * x; sxy += x * y; syy += y * y;
    }
    red[0][threadIdx.x] = sx; red[1][threadIdx.x] = sy; red[2][threadIdx.x] = sxx; red[3][threadIdx.x] = sxy; red[4][threadIdx.x] = syy;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
      if ((int)threadIdx.x < k)
#pragma unroll
        for (int q = 0; q < 5; ++q) red[q][threadIdx.x] += red[q][threadIdx.x + k];
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      const long long n = cvol;
      const long long Sx = (long long)red[0][0], Sy = (long long)red[1][0];
      const long long dxx = n * (long long)red[2][0] - Sx * Sx;   // n^2 var(x), n^2 cov(x, y), n^2 var(y): exact integers
      const long long dxy = n * (long long)red[3][0] - Sx * Sy;
      const long long dyy = n * (long long)red[4][0] - Sy * Sy;
      const double ybar = (double)Sy / (double)n;
      double slope = 0.0, icpt = ybar, rsq;
      if (dxx != 0) {
        slope = (double)dxy / (double)dxx;
        icpt = ybar - slope * (double)Sx / (double)n;
      }
      if (dyy == 0) rsq = 1.0;
      else if (dxx == 0) rsq = 0.0;
      else rsq = 1.0 - ((double)dyy - slope * (double)dxy) / (double)dyy;   // 1 - SSR / SST, both times n^2 / n
      reg[3 * (size_t)pair] = slope; reg[3 * (size_t)pair + 1] = icpt; reg[3 * (size_t)pair + 2] = rsq;
    }
  }
}

// ---- dense polynomial field -----------------------------------------------------------------------------------------
constexpr int POLY_MAXCOL = 20;   // columns of generate_polynomial_data for three coordinates, order 3
struct PolyArgs {
  double C[3][POLY_MAXCOL];
  int ncol[3];
  double ref[3];
};
__host__ __device__ inline int poly_cols(int order) { return order == 0 ? 1 : (order == 1 ? 4 : (order == 2 ? 10 : 20)); }

// the 20 columns at (v0, v1, v2): orders ascending, itertools.combinations_with_replacement order within one, every
// product built left to right from 1.0 (1 * v is exact)
__device__ __forceinline__ void monomials(double v0, double v1, double v2, double* m) {
  m[0] = 1.0; m[1] = v0; m[2] = v1; m[3] = v2;
  m[4] = v0 * v0; m[5] = v0 * v1; m[6] = v0 * v2; m[7] = v1 * v1; m[8] = v1 * v2; m[9] = v2 * v2;
  m[10] = m[4] * v0; m[11] = m[4] * v1; m[12] = m[4] * v2; m[13] = m[5] * v1; m[14] = m[5] * v2; m[15] = m[6] * v2;
  m[16] = m[7] * v1; m[17] = m[7] * v2; m[18] = m[8] * v2; m[19] = m[9] * v2;
}

// V consecutive y per thread: one 16-byte store per axis (V = 16 / sizeof(F)) where rows keep that alignment, else V = 1
template <class F, int V>
__global__ __launch_bounds__(256) void poly_field_k(PolyArgs p, int Z, int X, int Y, F* __restrict__ out) {
  const int y0 = (blockIdx.x * 256 + threadIdx.x) * V;
  if (y0 >= Y) return;
  const int x = blockIdx.y, z = blockIdx.z;
  const size_t vox = (size_t)Z * X * Y, o = ((size_t)z * X + x) * Y + y0;
  const double v0 = (double)z - p.ref[0], v1 = (double)x - p.ref[1];
  F res[3][V];
#pragma unroll
  for (int e = 0; e < V; ++e) {
    double m[POLY_MAXCOL];
    monomials(v0, v1, (double)(y0 + e) - p.ref[2], m);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      double s = p.C[a][0] * m[0];
#pragma unroll
      for (int k = 1; k < POLY_MAXCOL; ++k)
        if (k < p.ncol[a]) s = s + p.C[a][k] * m[k];
      res[a][e] = (F)s;
    }
  }
  if constexpr (V == 1) {
#pragma unroll
    for (int a = 0; a < 3; ++a) out[a * vox + o] = res[a][0];
  } else {
    typedef F vec __attribute__((ext_vector_type(V)));
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      vec q;
#pragma unroll
      for (int e = 0; e < V; ++e) q[e] = res[a][e];
      *(vec*)(out + a * vox + o) = q;
    }
  }
}

template <class F>
int poly_field_launch(const PolyArgs& p, int Z, int X, int Y, F* out) {
  constexpr int VEC = 16 / (int)sizeof(F);
  hipStream_t st = stream();
  ProfScope ps("poly_field");
  // a row starts on a 16-byte boundary of every plane set only if Y and the voxel count are multiples of VEC
  if (Y % VEC == 0)
    hipLaunchKernelGGL((poly_field_k<F, VEC>), dim3((unsigned)((Y / VEC + 255) / 256), (unsigned)X, (unsigned)Z), dim3(256), 0, st,
                       p, Z, X, Y, out);
  else
    hipLaunchKernelGGL((poly_field_k<F, 1>), dim3((unsigned)((Y + 255) / 256), (unsigned)X, (unsigned)Z), dim3(256), 0, st, p, Z, X,
                       Y, out);
  IA3_KCHECK();
  return IA3_OK;
}

// ---- bleedthrough profile ------------------------------------------------------------------------------------------
constexpr int BLEED_MAXC = 4;
constexpr int BLEED_MAXOFF = BLEED_MAXC * BLEED_MAXC - BLEED_MAXC;
// off-diagonal entries in row-major order of (tar, ref); an absent one (present == 0) has ncol 0 and stays 0.0
struct BleedArgs {
  double C[BLEED_MAXOFF][POLY_MAXCOL];
  int ncol;                      // columns of the fitting order
  unsigned char present[BLEED_MAXOFF];
  double ref[3];
};

// A (row-major N x N) <- its inverse by Gauss-Jordan elimination with partial pivoting, pivot = first row of largest
// magnitude in the column; false (A all NaN) where a pivot is zero or NaN.  Fully unrolled: A stays in registers.
template <int N>
__device__ __forceinline__ bool invert_gepp(double* A) {
  double B[N * N];
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = 0; j < N; ++j) B[i * N + j] = i == j ? 1.0 : 0.0;
  bool ok = true;
#pragma unroll
  for (int c = 0; c < N; ++c) {
    double best = fabs(A[c * N + c]);
    int piv = c;
#pragma unroll
    for (int r = c + 1; r < N; ++r) {
      const double v = fabs(A[r * N + c]);
      if (v > best) { best = v; piv = r; }
    }
#pragma unroll
    for (int r = c + 1; r < N; ++r) {   // (selects, not indexed moves: the rows stay in registers)
      const bool sw = piv == r;
#pragma unroll
      for (int j = 0; j < N; ++j) {
        const double a0 = A[c * N + j], a1 = A[r * N + j], b0 = B[c * N + j], b1 = B[r * N + j];
        A[c * N + j] = sw ? a1 : a0; A[r * N + j] = sw ? a0 : a1;
        B[c * N + j] = sw ? b1 : b0; B[r * N + j] = sw ? b0 : b1;
      }
    }
    const double p = A[c * N + c];
    ok = ok && (p != 0.0) && (p == p);
#pragma unroll
    for (int r = 0; r < N; ++r) {
      if (r == c) continue;
      const double f = A[r * N + c] / p;
#pragma unroll
      for (int j = 0; j < N; ++j) {
        A[r * N + j] = A[r * N + j] - f * A[c * N + j];
        B[r * N + j] = B[r * N + j] - f * B[c * N + j];
      }
    }
  }
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const double d = A[i * N + i];
#pragma unroll
    for (int j = 0; j < N; ++j) A[i * N + j] = ok ? B[i * N + j] / d : __builtin_nan("");
  }
  return ok;
}

// V consecutive y per thread, as poly_field_k.  MEANZ: the thread sums z = 0..Z-1 in order and divides by Z, output
// (N, N, X, Y); else blockIdx.z is z, output (N, N, Z, X, Y).
template <class F, int N, int V, bool MEANZ>
__global__ __launch_bounds__(256) void bleed_profile_k(BleedArgs p, int Z, int X, int Y, int invert, F* __restrict__ out,
                                                       unsigned long long* __restrict__ n_singular) {
  const int y0 = (blockIdx.x * 256 + threadIdx.x) * V;
  if (y0 >= Y) return;
  const int x = blockIdx.y;
  const size_t plane = MEANZ ? (size_t)X * Y : (size_t)Z * X * Y;
  const size_t o = MEANZ ? (size_t)x * Y + y0 : ((size_t)blockIdx.z * X + x) * Y + y0;
  const int zlo = MEANZ ? 0 : (int)blockIdx.z, zhi = MEANZ ? Z : (int)blockIdx.z + 1;
  const double v1 = (double)x - p.ref[1];
  double A[V][N * N];
#pragma unroll
  for (int e = 0; e < V; ++e)
#pragma unroll
    for (int q = 0; q < N * N; ++q) A[e][q] = 0.0;
  for (int z = zlo; z < zhi; ++z) {
    const double v0 = (double)z - p.ref[0];
#pragma unroll
    for (int e = 0; e < V; ++e) {
      double m[POLY_MAXCOL];
      monomials(v0, v1, (double)(y0 + e) - p.ref[2], m);
#pragma unroll
      for (int t = 0; t < N; ++t)
#pragma unroll
        for (int r = 0; r < N; ++r) {
          if (t == r) { A[e][t * N + r] = A[e][t * N + r] + 1.0; continue; }
          const int k0 = t * (N - 1) + (r < t ? r : r - 1);   // index among the off-diagonal entries
          double s = 0.0;
          if (p.present[k0]) {
            s = p.C[k0][0] * m[0];
#pragma unroll
            for (int k = 1; k < POLY_MAXCOL; ++k)
              if (k < p.ncol) s = s + p.C[k0][k] * m[k];
          }
          A[e][t * N + r] = A[e][t * N + r] + s;
        }
    }
  }
#pragma unroll
  for (int e = 0; e < V; ++e) {
    if constexpr (MEANZ) {
      const double dz = (double)Z;
#pragma unroll
      for (int q = 0; q < N * N; ++q) A[e][q] = A[e][q] / dz;
    }
    if (invert && !invert_gepp<N>(A[e])) atomicAdd(n_singular, 1ull);
  }
#pragma unroll
  for (int q = 0; q < N * N; ++q) {
    if constexpr (V == 1) {
      out[q * plane + o] = (F)A[0][q];
    } else {
      typedef F vec __attribute__((ext_vector_type(V)));
      vec w;
#pragma unroll
      for (int e = 0; e < V; ++e) w[e] = (F)A[e][q];
      *(vec*)(out + q * plane + o) = w;
    }
  }
}

template <class F, int N, bool MEANZ>
int bleed_profile_launch(const BleedArgs& p, int Z, int X, int Y, int invert, F* out, unsigned long long* n_singular) {
  // 16 bytes of a row per thread where the registers hold it.  In the z loop the compiler keeps the z-invariant products
  // (10 of the 20 columns per entry) in registers, N * N - N entries per pixel: N = 3 holds two pixels without scratch,
  // N = 4 one (kernel-resource-usage remarks of hipcc, gfx950)
  constexpr int FULL = 16 / (int)sizeof(F);
  constexpr int VEC = !MEANZ || N == 2 ? FULL : (N == 3 ? 2 : 1);
  hipStream_t st = stream();
  ProfScope ps("bleed_profile");
  const unsigned gz = MEANZ ? 1u : (unsigned)Z;
  // a vector store is aligned only if Y and with it every plane offset is a multiple of 16 bytes
  if (Y % (16 / (int)sizeof(F)) == 0)
    hipLaunchKernelGGL((bleed_profile_k<F, N, VEC, MEANZ>), dim3((unsigned)((Y / VEC + 255) / 256), (unsigned)X, gz), dim3(256), 0,
                       st, p, Z, X, Y, invert, out, n_singular);
  else
    hipLaunchKernelGGL((bleed_profile_k<F, N, 1, MEANZ>), dim3((unsigned)((Y + 255) / 256), (unsigned)X, gz), dim3(256), 0, st, p,
                       Z, X, Y, invert, out, n_singular);
  IA3_KCHECK();
  return IA3_OK;
}

template <class F, int N>
int bleed_profile_n(const BleedArgs& p, int Z, int X, int Y, int mean_z, int invert, F* out, unsigned long long* ns) {
  return mean_z ? bleed_profile_launch<F, N, true>(p, Z, X, Y, invert, out, ns)
                : bleed_profile_launch<F, N, false>(p, Z, X, Y, invert, out, ns);
}

template <class F>
int bleed_profile_t(const BleedArgs& p, int C, int Z, int X, int Y, int mean_z, int invert, F* out, unsigned long long* ns) {
  if (C == 2) return bleed_profile_n<F, 2>(p, Z, X, Y, mean_z, invert, out, ns);
  if (C == 3) return bleed_profile_n<F, 3>(p, Z, X, Y, mean_z, invert, out, ns);
  return bleed_profile_n<F, 4>(p, Z, X, Y, mean_z, invert, out, ns);
}

template <class T>
int crop_pairs_t(const ia3_stack* a, const ia3_stack* b, const double* ca, const double* cb, int n, const int* crop,
                 void* crops_a, void* crops_b, double* slope, double* icpt, double* rsq) {
  hipStream_t st = stream();
  const bool want_reg = slope || icpt || rsq;
  const size_t cvol = (size_t)crop[0] * crop[1] * crop[2];
  const size_t slab = (size_t)(crop[0] + 2 + 2 * NPAD) * (crop[1] + 2 + 2 * NPAD) * (crop[2] + 2 + 2 * NPAD);
  SplineTab tab;
  for (int len = PADLEN_MIN; len <= PADLEN_MAX; ++len) tab.q[len - PADLEN_MIN] = iir_init(len);
  // pairs per launch: slabs of at most 512 MB at a time
  const size_t fit = ((size_t)512 << 20) / (slab * sizeof(double));
  const int per = fit < (size_t)n ? (int)fit : n;
  const int ns = b ? 2 : 1;
  Scratch slabs((size_t)per * slab * sizeof(double)), cen((size_t)per * 3 * ns * sizeof(double)),
      boxes((size_t)per * cvol * ns * sizeof(T)), reg((size_t)per * 3 * sizeof(double));
  if (!slabs.p || !cen.p || !boxes.p || !reg.p) return IA3_ENOMEM;
  std::vector<double> hreg(want_reg ? (size_t)per * 3 : 0);
  for (int first = 0; first < n; first += per) {
    const int m = n - first < per ? n - first : per;
    double* dca = cen.as<double>();
    double* dcb = dca + (size_t)per * 3;
    T* oa = boxes.as<T>();
    T* ob = oa + (size_t)per * cvol;
    IA3_HIP(hipMemcpyAsync(dca, ca + 3 * (size_t)first, (size_t)m * 3 * sizeof(double), hipMemcpyHostToDevice, st));
    if (b) IA3_HIP(hipMemcpyAsync(dcb, cb + 3 * (size_t)first, (size_t)m * 3 * sizeof(double), hipMemcpyHostToDevice, st));
    {
      ProfScope ps("crop_pairs");
      hipLaunchKernelGGL((crop_pairs_k<T>), dim3((unsigned)m), dim3(256), 0, st, (const T*)a->d, b ? (const T*)b->d : (const T*)nullptr,
                         a->Z, a->X, a->Y, (const double*)dca, (const double*)dcb, crop[0], crop[1], crop[2], tab,
                         slabs.as<double>(), slab, oa, ob, want_reg ? reg.as<double>() : (double*)nullptr);
      IA3_KCHECK();
    }
    if (crops_a) IA3_HIP(hipMemcpyAsync((T*)crops_a + (size_t)first * cvol, oa, (size_t)m * cvol * sizeof(T), hipMemcpyDeviceToHost, st));
    if (b && crops_b) IA3_HIP(hipMemcpyAsync((T*)crops_b + (size_t)first * cvol, ob, (size_t)m * cvol * sizeof(T), hipMemcpyDeviceToHost, st));
    if (want_reg) IA3_HIP(hipMemcpyAsync(hreg.data(), reg.p, (size_t)m * 3 * sizeof(double), hipMemcpyDeviceToHost, st));
    IA3_HIP(hipStreamSynchronize(st));
    for (int i = 0; want_reg && i < m; ++i) {
      if (slope) slope[first + i] = hreg[3 * (size_t)i];
      if (icpt) icpt[first + i] = hreg[3 * (size_t)i + 1];
      if (rsq) rsq[first + i] = hreg[3 * (size_t)i + 2];
    }
  }
  return IA3_OK;
}

}  // namespace

extern "C" {

int ia3_crop_pairs_dev(const ia3_stack* a, const ia3_stack* b, const double* centers_a, const double* centers_b, int n,
                       const int* crop, void* crops_a_host, void* crops_b_host, double* slope, double* intercept,
                       double* rsq) {
  int rc = ensure_init(); if (rc) return rc;
  if (!a || !a->d || !centers_a || !crop || n < 0) return set_error(IA3_EINVAL, "null argument");
  if (a->dtype != IA3_U16 && a->dtype != IA3_F32) return set_error(IA3_EINVAL, "unsupported dtype code %d", a->dtype);
  const bool want_reg = slope || intercept || rsq;
  if (b) {
    if (!b->d || !centers_b) return set_error(IA3_EINVAL, "the second stack needs its centres");
    if (b->dtype != a->dtype || b->Z != a->Z || b->X != a->X || b->Y != a->Y)
      return set_error(IA3_EINVAL, "the two stacks must have the same shape and dtype");
  } else if (crops_b_host || want_reg) {
    return set_error(IA3_EINVAL, "boxes of a second stack and a regression need the second stack");
  }
  for (int k = 0; k < 3; ++k) {
    if (crop[k] < 1) return set_error(IA3_EINVAL, "crop size %d along axis %d: at least 1", crop[k], k);
    if (crop[k] > CROP_MAX) return set_error(IA3_EUNSUPPORTED, "crop size %d along axis %d: at most %d", crop[k], k, CROP_MAX);
  }
  if (want_reg && a->dtype != IA3_U16)
    return set_error(IA3_EUNSUPPORTED, "the regression of two boxes is built for uint16 stacks (exact integer sums)");
  const int dims[3] = {a->Z, a->X, a->Y};
  for (int i = 0; i < n; ++i)
    for (int s = 0; s < (b ? 2 : 1); ++s) {
      CropGeom g;
      if (!crop_geometry((s ? centers_b : centers_a) + 3 * (size_t)i, crop, dims, g))
        return set_error(IA3_EINVAL, "centre %d of stack %d: the crop does not meet the image", i, s);
    }
  if (n == 0) return IA3_OK;
  if (a->dtype == IA3_F32)
    return crop_pairs_t<float>(a, b, centers_a, centers_b, n, crop, crops_a_host, crops_b_host, slope, intercept, rsq);
  return crop_pairs_t<uint16_t>(a, b, centers_a, centers_b, n, crop, crops_a_host, crops_b_host, slope, intercept, rsq);
}

int ia3_poly_field_dev(const double* consts, const int* n_cols, const int* orders, const double* ref_center, int Z, int X,
                       int Y, int out_dtype, void** devptr) {
  int rc = ensure_init(); if (rc) return rc;
  if (!consts || !n_cols || !orders || !ref_center || !devptr) return set_error(IA3_EINVAL, "null argument");
  if (Z < 1 || X < 1 || Y < 1 || Z > 65535 || X > 65535) return set_error(IA3_EINVAL, "bad field shape (%d,%d,%d)", Z, X, Y);
  if (out_dtype != 1 && out_dtype != 2) return set_error(IA3_EINVAL, "field dtype must be float32 (1) or float64 (2)");
  PolyArgs p;
  const double* c = consts;
  for (int a = 0; a < 3; ++a) {
    if (orders[a] < 0) return set_error(IA3_EINVAL, "fitting order %d along axis %d", orders[a], a);
    if (orders[a] > 3) return set_error(IA3_EUNSUPPORTED, "fitting order %d along axis %d: orders 0 to 3 are built", orders[a], a);
    if (n_cols[a] != poly_cols(orders[a]))
      return set_error(IA3_EINVAL, "axis %d: order %d has %d columns, %d constants given", a, orders[a], poly_cols(orders[a]), n_cols[a]);
    p.ncol[a] = n_cols[a];
    for (int k = 0; k < POLY_MAXCOL; ++k) p.C[a][k] = k < n_cols[a] ? c[k] : 0.0;
    c += n_cols[a];
    p.ref[a] = ref_center[a];
  }
  const size_t bytes = (size_t)3 * Z * X * Y * (out_dtype == 1 ? 4 : 8);
  void* d = nullptr;
  rc = ia3_buffer_alloc(bytes, &d); if (rc) return rc;
  rc = out_dtype == 1 ? poly_field_launch<float>(p, Z, X, Y, (float*)d) : poly_field_launch<double>(p, Z, X, Y, (double*)d);
  if (!rc && hipStreamSynchronize(stream()) != hipSuccess) rc = set_error(IA3_EHIP, "polynomial field kernel failed");
  if (rc) { ia3_buffer_free(d); return rc; }
  *devptr = d;
  return IA3_OK;
}

int ia3_bleedthrough_profile_dev(const double* consts, const unsigned char* present, int C, int order,
                                 const double* ref_center, int Z, int X, int Y, int mean_z, int invert, int out_dtype,
                                 void** devptr, long long* n_singular) {
  int rc = ensure_init(); if (rc) return rc;
  if (!consts || !present || !ref_center || !devptr || !n_singular) return set_error(IA3_EINVAL, "null argument");
  if (C < 2 || order < 0) return set_error(IA3_EINVAL, "bad channel count %d or fitting order %d", C, order);
  if (C > BLEED_MAXC) return set_error(IA3_EUNSUPPORTED, "%d channels: 2 to %d are built", C, BLEED_MAXC);
  if (order > 3) return set_error(IA3_EUNSUPPORTED, "fitting order %d: orders 0 to 3 are built", order);
  if (Z < 1 || X < 1 || Y < 1 || Z > 65535 || X > 65535) return set_error(IA3_EINVAL, "bad profile shape (%d,%d,%d)", Z, X, Y);
  if (out_dtype != 1 && out_dtype != 2) return set_error(IA3_EINVAL, "profile dtype must be float32 (1) or float64 (2)");
  BleedArgs p;
  const int ncol = poly_cols(order);
  p.ncol = ncol;
  for (int k = 0; k < BLEED_MAXOFF; ++k) {
    p.present[k] = 0;
    for (int j = 0; j < POLY_MAXCOL; ++j) p.C[k][j] = 0.0;
  }
  for (int t = 0; t < C; ++t)
    for (int r = 0; r < C; ++r) {
      if (t == r) continue;
      const int k0 = t * (C - 1) + (r < t ? r : r - 1);
      p.present[k0] = present[t * C + r] ? 1 : 0;
      for (int j = 0; j < ncol; ++j) p.C[k0][j] = consts[(size_t)(t * C + r) * ncol + j];
    }
  for (int a = 0; a < 3; ++a) p.ref[a] = ref_center[a];
  const size_t bytes = (size_t)C * C * (mean_z ? 1 : Z) * X * Y * (out_dtype == 1 ? 4 : 8);
  Scratch cnt(sizeof(unsigned long long));
  if (!cnt.p) return IA3_ENOMEM;
  hipStream_t st = stream();
  IA3_HIP(hipMemsetAsync(cnt.p, 0, sizeof(unsigned long long), st));
  void* d = nullptr;
  rc = ia3_buffer_alloc(bytes, &d); if (rc) return rc;
  unsigned long long* ns = cnt.as<unsigned long long>();
  rc = out_dtype == 1 ? bleed_profile_t<float>(p, C, Z, X, Y, mean_z, invert, (float*)d, ns)
                      : bleed_profile_t<double>(p, C, Z, X, Y, mean_z, invert, (double*)d, ns);
  unsigned long long h = 0;
  if (!rc && (hipMemcpyAsync(&h, cnt.p, sizeof(h), hipMemcpyDeviceToHost, st) != hipSuccess ||
              hipStreamSynchronize(st) != hipSuccess))
    rc = set_error(IA3_EHIP, "bleedthrough profile kernel failed");
  if (rc) { ia3_buffer_free(d); return rc; }
  *n_singular = (long long)h;
  *devptr = d;
  return IA3_OK;
}

}  // extern "C"
