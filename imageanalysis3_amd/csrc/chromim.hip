// The chromosome image of a field of view (reference: classes/field_of_view.py:1821-1917
// Field_of_View._generate_chrom_im_from_data): the float64 sum of the resident uint16 stacks of every processed round,
// the unwarped ones shifted by their rounded drift and filled up with their whole-stack median.
//   chrom_add_k     up to 16 stacks into the float64 volume in one launch: each thread owns 8 consecutive y voxels of one
//                   (z, x) row, reads them from every image and does one read-modify-write of its 64 bytes
//   ia3_select.h    np.median of a stack (the radix select that corrections.hip, stats.hip and morph.hip use as well)
// Every term and every partial sum is a multiple of 0.5 far below 2^52: the sums are exact, whatever the order of the
// images and of the operations, and the same on every run.  No atomics, no LDS.
#include "ia3_rt.h"
#include "ia3_select.h"
#include <limits.h>

using namespace ia3rt;

namespace {

constexpr int BATCH = 16;   // images of a launch
constexpr int RUN = 8;      // voxels of a thread: 64 B of the float64 volume, 16 B of an image

struct AddImage {
  const uint16_t* p;
  int dz, dx, dy;   // out[j] += im[j + d] where that is inside, bg elsewhere
  int pad;
  double bg;
};
struct AddBatch {
  AddImage im[BATCH];
  int n;
};

// the 8 values at elements off .. off + 7 of the 16 that the two aligned blocks lo, hi hold
template <int OFF>
__device__ __forceinline__ void take8(const uint4& lo, const uint4& hi, unsigned short* v) {
  const unsigned w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
  for (int j = 0; j < RUN; ++j) {
    const int e = OFF + j;
    v[j] = (unsigned short)((e & 1) ? w[e >> 1] >> 16 : w[e >> 1] & 0xFFFFu);
  }
}

// Rows of a multiple of 8 voxels, every pointer 16-byte aligned: the run of the volume is four aligned 16-byte accesses
// each way, the run of an image the two aligned 16-byte blocks that cover its dy-shifted voxels (blocks outside the row
// are not read), picked apart with compile-time indices (dy mod 8 is the same for the whole launch).
// runs = Z * X * (Y / 8) < 2^31, so the grid-stride index does not wrap.
__global__ __launch_bounds__(256) void chrom_add_k(double* __restrict__ acc, int Z, int X, int Y, unsigned runs, AddBatch b) {
  const unsigned rw = (unsigned)Y / RUN;
  for (unsigned r = blockIdx.x * 256u + threadIdx.x; r < runs; r += gridDim.x * 256u) {
    const unsigned row = r / rw;
    const int y0 = (int)(r - row * rw) * RUN;
    const int z = (int)(row / (unsigned)X), x = (int)(row - (unsigned)z * (unsigned)X);
    double2* dst = (double2*)(acc + (size_t)row * Y + y0);
    double2 a0 = dst[0], a1 = dst[1], a2 = dst[2], a3 = dst[3];
    double s[RUN] = {a0.x, a0.y, a1.x, a1.y, a2.x, a2.y, a3.x, a3.y};
    for (int k = 0; k < b.n; ++k) {
      const AddImage im = b.im[k];
      const int sz = z + im.dz, sx = x + im.dx;
      if (sz < 0 || sz >= Z || sx < 0 || sx >= X) {   // the row lies outside the image's crop
#pragma unroll
        for (int j = 0; j < RUN; ++j) s[j] += im.bg;
        continue;
      }
      const int sy = y0 + im.dy;                      // first source voxel, anywhere in (-Y, 2 Y)
      const int blk = sy >> 3, off = sy & 7;          // arithmetic shift: floor
      const uint4* src = (const uint4*)(im.p + ((size_t)sz * X + sx) * Y);
      uint4 lo = make_uint4(0, 0, 0, 0), hi = lo;
      if (blk >= 0 && blk < (int)rw) lo = src[blk];
      if (off && blk + 1 >= 0 && blk + 1 < (int)rw) hi = src[blk + 1];
      unsigned short v[RUN];
      switch (off) {
        case 0: take8<0>(lo, hi, v); break;
        case 1: take8<1>(lo, hi, v); break;
        case 2: take8<2>(lo, hi, v); break;
        case 3: take8<3>(lo, hi, v); break;
        case 4: take8<4>(lo, hi, v); break;
        case 5: take8<5>(lo, hi, v); break;
        case 6: take8<6>(lo, hi, v); break;
        default: take8<7>(lo, hi, v); break;
      }
#pragma unroll
      for (int j = 0; j < RUN; ++j) s[j] += (unsigned)(sy + j) < (unsigned)Y ? (double)v[j] : im.bg;
    }
    dst[0] = make_double2(s[0], s[1]);
    dst[1] = make_double2(s[2], s[3]);
    dst[2] = make_double2(s[4], s[5]);
    dst[3] = make_double2(s[6], s[7]);
  }
}

// any row length and alignment: the same runs (the last of a row may be short), one voxel at a time
__global__ __launch_bounds__(256) void chrom_add_any_k(double* __restrict__ acc, int Z, int X, int Y, unsigned runs, AddBatch b) {
  const unsigned rw = ((unsigned)Y + RUN - 1) / RUN;
  for (unsigned r = blockIdx.x * 256u + threadIdx.x; r < runs; r += gridDim.x * 256u) {
    const unsigned row = r / rw;
    const int y0 = (int)(r - row * rw) * RUN;
    const int z = (int)(row / (unsigned)X), x = (int)(row - (unsigned)z * (unsigned)X);
    double* dst = acc + (size_t)row * Y + y0;
    const int len = Y - y0 < RUN ? Y - y0 : RUN;
    double s[RUN];
#pragma unroll
    for (int j = 0; j < RUN; ++j) s[j] = j < len ? dst[j] : 0.0;
    for (int k = 0; k < b.n; ++k) {
      const AddImage im = b.im[k];
      const int sz = z + im.dz, sx = x + im.dx;
      const bool in = sz >= 0 && sz < Z && sx >= 0 && sx < X;
      const uint16_t* src = im.p + (in ? ((size_t)sz * X + sx) * Y : 0);
      const int sy = y0 + im.dy;
#pragma unroll
      for (int j = 0; j < RUN; ++j) s[j] += in && j < len && (unsigned)(sy + j) < (unsigned)Y ? (double)src[sy + j] : im.bg;
    }
#pragma unroll
    for (int j = 0; j < RUN; ++j)
      if (j < len) dst[j] = s[j];
  }
}

int check_handle(const ia3_chrom_image* h) {
  if (!h || !h->d) return set_error(IA3_EINVAL, "null chromosome image");
  return IA3_OK;
}

int add_batch(ia3_chrom_image* h, const AddBatch& b) {
  const bool aligned = h->Y % RUN == 0 && ((uintptr_t)h->d & 15) == 0;
  bool fast = aligned;
  for (int k = 0; k < b.n; ++k) fast = fast && ((uintptr_t)b.im[k].p & 15) == 0;
  const size_t runs = (size_t)h->Z * h->X * (((size_t)h->Y + RUN - 1) / RUN);
  size_t blocks = (runs + 255) / 256, bound = (size_t)num_cus() * 8;
  if (blocks > bound) blocks = bound;
  ProfScope ps("chrom_add");
  if (fast) hipLaunchKernelGGL(chrom_add_k, dim3((unsigned)blocks), dim3(256), 0, stream(), h->d, h->Z, h->X, h->Y, (unsigned)runs, b);
  else hipLaunchKernelGGL(chrom_add_any_k, dim3((unsigned)blocks), dim3(256), 0, stream(), h->d, h->Z, h->X, h->Y, (unsigned)runs, b);
  IA3_KCHECK();
  return IA3_OK;
}

}  // namespace

extern "C" {

int ia3_chrom_image_create(int Z, int X, int Y, ia3_chrom_image** out) {
  int rc = ensure_init(); if (rc) return rc;
  if (!out) return set_error(IA3_EINVAL, "null output");
  if (Z < 1 || X < 1 || Y < 1) return set_error(IA3_EINVAL, "bad chromosome image shape (%d,%d,%d)", Z, X, Y);
  const size_t runs = (size_t)Z * X * (((size_t)Y + RUN - 1) / RUN);
  if (Z > INT_MAX / 2 || runs > (size_t)INT_MAX) return set_error(IA3_EUNSUPPORTED, "chromosome images of up to 2^31 - 1 runs of 8 voxels are built");
  ia3_stack* store = nullptr;
  rc = ia3_stack_alloc(IA3_F32, 2 * Z, X, Y, &store); if (rc) return rc;   // Z * X * Y * 8 bytes
  ia3_chrom_image* h = new ia3_chrom_image{store, (double*)store->d, Z, X, Y, (size_t)Z * X * Y};
  hipError_t e = hipMemsetAsync(h->d, 0, h->n * sizeof(double), stream());
  if (e == hipSuccess) e = hipStreamSynchronize(stream());
  if (e != hipSuccess) {
    ia3_chrom_image_free(h);
    return set_error(IA3_EHIP, "clearing the chromosome image failed: %s", hipGetErrorString(e));
  }
  *out = h;
  return IA3_OK;
}

void ia3_chrom_image_free(ia3_chrom_image* h) {
  if (!h) return;
  ia3_stack_free(h->store);
  delete h;
}

int ia3_chrom_image_upload(ia3_chrom_image* h, const double* host) {
  int rc = ensure_init(); if (rc) return rc;
  rc = check_handle(h); if (rc) return rc;
  if (!host) return set_error(IA3_EINVAL, "null host array");
  IA3_HIP(hipMemcpyAsync(h->d, host, h->n * sizeof(double), hipMemcpyHostToDevice, stream()));
  IA3_HIP(hipStreamSynchronize(stream()));
  return IA3_OK;
}

int ia3_chrom_image_download(const ia3_chrom_image* h, double* host) {
  int rc = ensure_init(); if (rc) return rc;
  rc = check_handle(h); if (rc) return rc;
  if (!host) return set_error(IA3_EINVAL, "null host array");
  IA3_HIP(hipMemcpyAsync(host, h->d, h->n * sizeof(double), hipMemcpyDeviceToHost, stream()));
  IA3_HIP(hipStreamSynchronize(stream()));
  return IA3_OK;
}

int ia3_stack_median_dev(const ia3_stack* s, double* out) {
  int rc = ensure_init(); if (rc) return rc;
  if (!s || !s->d || !out) return set_error(IA3_EINVAL, "null argument");
  if (s->dtype != IA3_U16 && s->dtype != IA3_F32) return set_error(IA3_EINVAL, "stack dtype must be uint16 or float32");
  if (s->Z < 1 || s->X < 1 || s->Y < 1) return set_error(IA3_EINVAL, "empty stack");
  std::vector<double> med;
  rc = host_medians("morph_select", s->d, s->dtype, 1, (size_t)s->Z * s->X * s->Y, med); if (rc) return rc;
  *out = med[0];
  return IA3_OK;
}

int ia3_chrom_image_add_dev(ia3_chrom_image* h, const ia3_stack* const* ims, const int* flags, const int* shifts, int n,
                            double* backgrounds_out) {
  int rc = ensure_init(); if (rc) return rc;
  rc = check_handle(h); if (rc) return rc;
  if (n < 0 || (n > 0 && (!ims || !flags || !shifts))) return set_error(IA3_EINVAL, "null argument");
  const int N[3] = {h->Z, h->X, h->Y};
  for (int k = 0; k < n; ++k) {
    const ia3_stack* s = ims[k];
    if (!s || !s->d) return set_error(IA3_EINVAL, "image %d: null stack", k);
    if (s->dtype != IA3_U16) return set_error(IA3_EUNSUPPORTED, "image %d: the chromosome image is built from uint16 stacks (dtype code %d given)", k, s->dtype);
    if (s->Z != h->Z || s->X != h->X || s->Y != h->Y)
      return set_error(IA3_EINVAL, "image %d has the shape (%d,%d,%d), the chromosome image (%d,%d,%d)", k, s->Z, s->X, s->Y, h->Z, h->X, h->Y);
    if (flags[k] == 2) continue;
    for (int a = 0; a < 3; ++a) {
      const long long d = shifts[3 * k + a];
      if (d >= N[a] || -d >= N[a])
        return set_error(IA3_EINVAL, "image %d: shift %lld along axis %d of length %d: operands could not be broadcast together", k, d, a, N[a]);
    }
  }
  std::vector<double> bg((size_t)n, 0.0);
  for (int k = 0; k < n; ++k) {
    if (flags[k] == 2) continue;
    std::vector<double> med;
    rc = host_medians("morph_select", ims[k]->d, IA3_U16, 1, h->n, med); if (rc) return rc;
    bg[k] = med[0];
  }
  if (backgrounds_out)
    for (int k = 0; k < n; ++k) backgrounds_out[k] = bg[k];
  for (int first = 0; first < n; first += BATCH) {
    AddBatch b;
    memset(&b, 0, sizeof b);
    b.n = n - first < BATCH ? n - first : BATCH;
    for (int i = 0; i < b.n; ++i) {
      const int k = first + i;
      const bool warped = flags[k] == 2;
      b.im[i].p = (const uint16_t*)ims[k]->d;
      b.im[i].dz = warped ? 0 : shifts[3 * k];
      b.im[i].dx = warped ? 0 : shifts[3 * k + 1];
      b.im[i].dy = warped ? 0 : shifts[3 * k + 2];
      b.im[i].bg = bg[k];
    }
    rc = add_batch(h, b); if (rc) return rc;
  }
  IA3_HIP(hipStreamSynchronize(stream()));
  return IA3_OK;
}

}  // extern "C"
