// Density clouds of traced chromosomes on the device: visual_tools.py:68-72 gauss_ker, :87-116 add_source and
// the loop of structure_tools/chromosome.py:5-57 over the loci of a homolog.  The reference pastes one (s + 1)**3 Gaussian
// box per source into the image; here every voxel gathers the sources that reach it, in their given order.
//   cloud_k     a workgroup owns a CL_T0 x CL_T1 x CL_T2 tile of one image, one voxel per lane, the last axis across lanes.
//               The image's sources pass through LDS CL_CHUNK at a time: the first wave takes one source per lane, works out
//               its box (ia3_cloud.h) and keeps it when the box meets the tile; the kept ones are packed in order with a
//               ballot and a prefix count.  Then the workgroup fills, per kept source, the CL_TERMS values u * u of the
//               tile's coordinates on the three axes (CL_OUT for a coordinate outside the source's box), and a lane adds
//               exp(-((T1[x] + T2[y]) + T0[z]) / 2.) * h for the sources whose box holds its voxel: the value of the
//               reference's kernel at that voxel bit for bit up to exp, because each term depends on one coordinate only.
//   kernel_k    a bare gauss_ker, one lane per value.
// Two ways to accumulate: float64 (add_source), or float32 rounded after every source (what assigning add_source's result
// into a float32 slice does, chromosome.py:35).  LDS: 18 KiB per workgroup of four waves.  No atomics and no dependence on
// the launch shape: a voxel sees the sources of its image in order whatever the other images of the call are.
#include "ia3_rt.h"
#include "ia3_cloud.h"
#include <math.h>
#include <string.h>
#include <vector>

using namespace ia3rt;
using namespace ia3cl;

namespace {

struct ClStage {       // a kept source of the chunk
  ClBox box;
  int s;
  double h, disp[3], sig[3];
};

struct ClArgs {
  const double* src;        // n_sources x 8: pos[3], h, sig[3], size_fold
  const int* image_start;   // n_images + 1
  int shape[3];
  int tiles1, tiles2;       // tiles along the axes 1 and 2
  void* images;             // n_images x shape, float64 or float32
};

template <bool F32>
__global__ __launch_bounds__(CL_THREADS) void cloud_k(ClArgs A) {
  __shared__ ClStage st[CL_CHUNK];
  __shared__ double terms[CL_CHUNK][CL_TERMS];
  __shared__ int n_kept;
  const int tid = threadIdx.x;
  const int l2 = tid % CL_T2, l1 = (tid / CL_T2) % CL_T1, l0 = tid / (CL_T2 * CL_T1);
  const int tile = blockIdx.x, img = blockIdx.y;
  const int o2 = (tile % A.tiles2) * CL_T2, o1 = ((tile / A.tiles2) % A.tiles1) * CL_T1, o0 = (tile / (A.tiles2 * A.tiles1)) * CL_T0;
  const int origin[3] = {o0, o1, o2};
  const int extent[3] = {CL_T0, CL_T1, CL_T2};
  const int v0 = o0 + l0, v1 = o1 + l1, v2 = o2 + l2;
  const bool live = v0 < A.shape[0] && v1 < A.shape[1] && v2 < A.shape[2];
  const size_t at = (((size_t)img * A.shape[0] + v0) * A.shape[1] + v1) * A.shape[2] + v2;
  double acc = 0.0;
  float acc32 = 0.0f;
  if (live) {
    if (F32) acc32 = ((const float*)A.images)[at];
    else acc = ((const double*)A.images)[at];
  }
  const int j_end = A.image_start[img + 1];
  for (int j0 = A.image_start[img]; j0 < j_end; j0 += CL_CHUNK) {
    if (tid < CL_CHUNK) {   // the first wave: one source per lane
      const int j = j0 + tid;
      ClStage t;
      bool hit = false;
      if (j < j_end) {
        const double* r = A.src + (size_t)j * 8;
        int s = 0;
        if (cl_size(r[4], r[5], r[6], r[7], &s) == 0) {   // the host refused every other source before the launch
          hit = cl_box(r, s, A.shape, &t.box);
          for (int k = 0; k < 3; ++k) hit = hit && t.box.lo[k] < origin[k] + extent[k] && t.box.hi[k] > origin[k];
          t.s = s;
          t.h = r[3];
          for (int k = 0; k < 3; ++k) { t.disp[k] = cl_disp(r[k]); t.sig[k] = r[4 + k]; }
        }
      }
      const unsigned long long kept = __ballot(hit);
      if (hit) st[__popcll(kept & ((1ull << tid) - 1ull))] = t;   // in order
      if (tid == 0) n_kept = __popcll(kept);
    }
    __syncthreads();
    const int n = n_kept;
    for (int i = tid; i < n * CL_TERMS; i += CL_THREADS) {
      const int j = i / CL_TERMS, e = i % CL_TERMS;
      const int axis = e < CL_T0 ? 0 : (e < CL_T0 + CL_T1 ? 1 : 2);
      const int off = axis == 0 ? e : (axis == 1 ? e - CL_T0 : e - CL_T0 - CL_T1);
      const int p = cl_pair(axis), at_axis = origin[axis] + off;
      const bool in_box = at_axis >= st[j].box.lo[axis] && at_axis < st[j].box.hi[axis];
      terms[j][e] = in_box ? cl_term((long long)at_axis - st[j].box.pmin[axis], st[j].disp[p], st[j].s, st[j].sig[p]) : CL_OUT;
    }
    __syncthreads();
    if (live) {
      for (int j = 0; j < n; ++j) {
        const double t0 = terms[j][l0], t1 = terms[j][CL_T0 + l1], t2 = terms[j][CL_T0 + CL_T1 + l2];
        if (cl_out(t0) || cl_out(t1) || cl_out(t2)) continue;   // the box of the source does not hold the voxel
        const double t = cl_arg(t0, t1, t2);
        const double e = t < CL_CUT ? 0.0 : exp(t);   // a NaN argument (sigma 0 at the centre) stays NaN
        if (F32) acc32 = (float)((double)acc32 + e * st[j].h);
        else acc = acc + e * st[j].h;
      }
    }
    __syncthreads();
  }
  if (!live) return;
  if (F32) ((float*)A.images)[at] = acc32;
  else ((double*)A.images)[at] = acc;
}

__global__ void kernel_k(double sig0, double sig1, double sig2, double d0, double d1, double d2, int s, double* out) {
  const long long n = (long long)s + 1, i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * n * n) return;
  const long long c = i % n, b = (i / n) % n, a = i / (n * n);
  const double t = cl_arg(cl_term(a, d2, s, sig2), cl_term(b, d0, s, sig0), cl_term(c, d1, s, sig1));
  out[i] = t < CL_CUT ? 0.0 : exp(t);
}

// what both forms refuse before any launch
int check_call(const char* who, const double* sources, const int* image_start, int n_images, int d0, int d1, int d2, int mode) {
  if (mode != IA3_CLOUD_F64 && mode != IA3_CLOUD_F32) return set_error(IA3_EINVAL, "%s: mode %d", who, mode);
  if (n_images < 1 || n_images > IA3_CLOUD_MAX_IMAGES || !image_start || image_start[0] != 0)
    return set_error(IA3_EINVAL, "%s: %d images (1 to %d), or a table that does not start at 0", who, n_images, IA3_CLOUD_MAX_IMAGES);
  if (d0 < 1 || d1 < 1 || d2 < 1 || d0 > IA3_CLOUD_MAX_DIM || d1 > IA3_CLOUD_MAX_DIM || d2 > IA3_CLOUD_MAX_DIM)
    return set_error(IA3_EINVAL, "%s: an image of %d x %d x %d (1 to %d along an axis)", who, d0, d1, d2, IA3_CLOUD_MAX_DIM);
  for (int i = 0; i < n_images; ++i)
    if (image_start[i + 1] < image_start[i]) return set_error(IA3_EINVAL, "%s: image_start falls at image %d", who, i);
  const int n = image_start[n_images];
  if (n > 0 && !sources) return set_error(IA3_EINVAL, "%s: null source table", who);
  for (int j = 0; j < n; ++j) {
    const double* r = sources + (size_t)j * 8;
    int s = 0;
    const int bad = cl_size(r[4], r[5], r[6], r[7], &s);
    if (bad == 1 || !isfinite(r[0]) || !isfinite(r[1]) || !isfinite(r[2]))
      return set_error(IA3_EINVAL, "%s: source %d has a position, sigma or size_fold that is not finite", who, j);
    if (bad) return set_error(IA3_EINVAL, "%s: source %d has a box of int(%g * %g) + 1, outside 1 to %d", who, j,
                              fmax(fmax(r[4], r[5]), r[6]), r[7], IA3_CLOUD_MAX_S + 1);
  }
  return IA3_OK;
}

// the device copies of a call's two tables; the entry that makes them keeps them until its last synchronise
struct ClTables {
  Scratch src, start;
  ClTables(int n, int n_images) : src((size_t)(n > 0 ? n : 1) * 8 * sizeof(double)), start(((size_t)n_images + 1) * sizeof(int)) {}
};

// queues the uploads of the tables and the kernel; the caller synchronises
int launch(const ClTables& T, const double* sources, const int* image_start, int n_images, int d0, int d1, int d2, int mode,
           void* d_images) {
  const int n = image_start[n_images];
  if (n == 0) return IA3_OK;
  if (!T.src.p || !T.start.p) return set_error(IA3_ENOMEM, "cloud_render: scratch for %d sources", n);
  hipStream_t st = stream();
  IA3_HIP(hipMemcpyAsync(T.src.p, sources, (size_t)n * 8 * sizeof(double), hipMemcpyHostToDevice, st));
  IA3_HIP(hipMemcpyAsync(T.start.p, image_start, ((size_t)n_images + 1) * sizeof(int), hipMemcpyHostToDevice, st));
  ClArgs A;
  A.src = T.src.as<double>(); A.image_start = T.start.as<int>();
  A.shape[0] = d0; A.shape[1] = d1; A.shape[2] = d2;
  const long long t0 = (d0 + CL_T0 - 1) / CL_T0;
  A.tiles1 = (d1 + CL_T1 - 1) / CL_T1; A.tiles2 = (d2 + CL_T2 - 1) / CL_T2;
  A.images = d_images;
  const long long tiles = t0 * A.tiles1 * A.tiles2;
  if (tiles > 2147483647LL) return set_error(IA3_EINVAL, "cloud_render: %lld tiles", tiles);
  ProfScope ps("cloud");
  if (mode == IA3_CLOUD_F32) hipLaunchKernelGGL(cloud_k<true>, dim3((unsigned)tiles, (unsigned)n_images), dim3(CL_THREADS), 0, st, A);
  else hipLaunchKernelGGL(cloud_k<false>, dim3((unsigned)tiles, (unsigned)n_images), dim3(CL_THREADS), 0, st, A);
  IA3_KCHECK();
  return IA3_OK;
}

}  // namespace

extern "C" {

int ia3_cloud_render_dev(const double* sources, const int* image_start, int n_images, int d0, int d1, int d2, int mode,
                         int zero_first, void* d_images) {
  int rc = check_call("cloud_render_dev", sources, image_start, n_images, d0, d1, d2, mode); if (rc) return rc;
  if (!d_images) return set_error(IA3_EINVAL, "cloud_render_dev: null images");
  rc = ensure_init(); if (rc) return rc;
  const size_t bytes = (size_t)n_images * d0 * d1 * d2 * (mode == IA3_CLOUD_F32 ? sizeof(float) : sizeof(double));
  if (zero_first) IA3_HIP(hipMemsetAsync(d_images, 0, bytes, stream()));
  ClTables T(image_start[n_images], n_images);
  rc = launch(T, sources, image_start, n_images, d0, d1, d2, mode, d_images);
  // the images have been written when the call returns; the tables are the caller's and the scratch goes back
  const hipError_t e = hipStreamSynchronize(stream());
  if (rc) return rc;
  IA3_HIP(e);
  return IA3_OK;
}

int ia3_cloud_render(const double* sources, const int* image_start, int n_images, int d0, int d1, int d2, int mode,
                     const void* init, void* out) {
  int rc = check_call("cloud_render", sources, image_start, n_images, d0, d1, d2, mode); if (rc) return rc;
  if (!out) return set_error(IA3_EINVAL, "cloud_render: null output");
  rc = ensure_init(); if (rc) return rc;
  const size_t bytes = (size_t)n_images * d0 * d1 * d2 * (mode == IA3_CLOUD_F32 ? sizeof(float) : sizeof(double));
  Scratch d_im(bytes);
  if (!d_im.p) return set_error(IA3_ENOMEM, "cloud_render: %zu bytes of images", bytes);
  hipStream_t st = stream();
  if (init) IA3_HIP(hipMemcpyAsync(d_im.p, init, bytes, hipMemcpyHostToDevice, st));
  else IA3_HIP(hipMemsetAsync(d_im.p, 0, bytes, st));
  ClTables T(image_start[n_images], n_images);
  rc = launch(T, sources, image_start, n_images, d0, d1, d2, mode, d_im.p);
  hipError_t e = rc ? hipSuccess : hipMemcpyAsync(out, d_im.p, bytes, hipMemcpyDeviceToHost, st);
  const hipError_t e2 = hipStreamSynchronize(st);   // the one wait of the call, also on an error: the scratch goes back after it
  if (rc) return rc;
  IA3_HIP(e);
  IA3_HIP(e2);
  return IA3_OK;
}

int ia3_cloud_gauss_ker(const double* sig, int s, const double* disp, double* out) {
  if (!sig || !disp || !out) return set_error(IA3_EINVAL, "cloud_gauss_ker: null sigmas, displacements or output");
  if (s < 0 || s > IA3_CLOUD_MAX_KER_S) return set_error(IA3_EINVAL, "cloud_gauss_ker: sxyz %d (0 to %d)", s, IA3_CLOUD_MAX_KER_S);
  int rc = ensure_init(); if (rc) return rc;
  const size_t n = (size_t)(s + 1) * (s + 1) * (s + 1);
  Scratch d_out(n * sizeof(double));
  if (!d_out.p) return set_error(IA3_ENOMEM, "cloud_gauss_ker: %zu values", n);
  hipStream_t st = stream();
  hipLaunchKernelGGL(kernel_k, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, sig[0], sig[1], sig[2], disp[0], disp[1], disp[2],
                     s, d_out.as<double>());
  IA3_KCHECK();
  IA3_HIP(hipMemcpyAsync(out, d_out.p, n * sizeof(double), hipMemcpyDeviceToHost, st));
  IA3_HIP(hipStreamSynchronize(st));
  return IA3_OK;
}

}  // extern "C"
