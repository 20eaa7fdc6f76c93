// Segmentation label images on the device: everything that pairs a spot table or a resident stack with
// a uint16 label stack, in integer arithmetic, so every result is the reference's bit for bit and the same on every run.
//   label_boxes_k    one streaming pass: voxel count and tight bounds of every label 1..L
//                    (segmentation_tools/cell.py:598-611 segmentation_mask_2_bounding_box, for all cells at once)
//   cube_labels_k    per spot, over the clamped (2r+1)^3 cube around its rounded centre: the most frequent positive label
//                    (classes/partition_spots.py:113-140 spots_to_labels) or whether a given label occurs
//   cube_max_k       per spot the largest value of the cube (:143-157 spots_to_DAPI)
//   cube_gather_k    the whole (N, (2r+1)^3) matrix (:212-236 find_coordinate_intensities)
// The index arithmetic is csrc/ia3_labels.h, which tests/native/labels_cpu.cpp builds for the host.
#include "ia3_rt.h"
#include "ia3_labels.h"
#include <limits.h>

using namespace ia3rt;

namespace {
using namespace ia3lab;

// ---- label_boxes_k ---------------------------------------------------------------------------------------------------
// A table row is [count, zmin, zmax, xmin, xmax, ymin, ymax] while it is accumulated (count 0, minima INT_MAX, maxima -1
// when empty); label_table_finish_k turns it into [count, z0, z1, x0, x1, y0, y1] with [start, stop) bounds.
constexpr int ROW = 7;
constexpr int BOX_THREADS = 256;
constexpr int BOX_VEC = 8;                        // voxels of one 16-byte load
constexpr int BOX_TILE = BOX_THREADS * BOX_VEC;   // voxels staged in LDS per step
constexpr int BOX_WAVE = BOX_TILE / (BOX_THREADS / 64);   // ... of which every wavefront takes 512, 64 at a time
constexpr int BOX_SLOTS = 512;                    // labels a workgroup combines in LDS before it goes to the global table
constexpr int BOX_SLOT_BITS = 9;
constexpr int BOX_PROBES = 8;

__global__ void label_table_init_k(int* __restrict__ t, int rows) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows) return;
  int* r = t + (size_t)i * ROW;
  r[0] = 0;
  r[1] = INT_MAX; r[2] = -1; r[3] = INT_MAX; r[4] = -1; r[5] = INT_MAX; r[6] = -1;
}

__global__ void label_table_finish_k(int* __restrict__ t, int rows) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows) return;
  int* r = t + (size_t)i * ROW;
  if (i == 0 || r[0] == 0) {
    for (int k = 0; k < ROW; ++k) r[k] = 0;
  } else {
    r[2] += 1; r[4] += 1; r[6] += 1;
  }
}

// minima only fall and maxima only rise: a value that would not move the entry needs no atomic
__device__ inline void global_row_update(int* __restrict__ r, int cnt, int z0, int z1, int x0, int x1, int y0, int y1) {
  volatile int* v = r;
  atomicAdd(r, cnt);
  if (v[1] > z0) atomicMin(r + 1, z0);
  if (v[2] < z1) atomicMax(r + 2, z1);
  if (v[3] > x0) atomicMin(r + 3, x0);
  if (v[4] < x1) atomicMax(r + 4, x1);
  if (v[5] > y0) atomicMin(r + 5, y0);
  if (v[6] < y1) atomicMax(r + 6, y1);
}

// One pass over the n voxels of a (., X, Y) uint16 stack.  A workgroup takes a contiguous range of tiles; a tile comes in
// with 16-byte loads and is read back from LDS 64 consecutive voxels per wavefront at a time.  Labels are piecewise
// constant along a row: the lanes where a run begins (first lane, a change of label, a new row) are found with one
// ballot, and only those lanes (of a label in 1..L) update anything, with the length of their run.  The update goes to
// the workgroup's LDS table of the labels it has met (open addressing, BOX_PROBES probes) and to the global table only
// when that is full; the LDS table is added to the global one once, at the end.  Integer atomics throughout: the result
// does not depend on the order of arrival.
__global__ __launch_bounds__(BOX_THREADS) void label_boxes_k(const uint16_t* __restrict__ lab, unsigned n, int X, int Y, int L,
                                                              int aligned, unsigned tiles_per_block, int* __restrict__ table) {
  __shared__ __attribute__((aligned(16))) uint16_t s_vox[BOX_TILE];
  __shared__ int s_key[BOX_SLOTS];
  __shared__ int s_val[BOX_SLOTS * ROW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < BOX_SLOTS; i += BOX_THREADS) {
    s_key[i] = 0;
    int* r = s_val + i * ROW;
    r[0] = 0;
    r[1] = INT_MAX; r[2] = -1; r[3] = INT_MAX; r[4] = -1; r[5] = INT_MAX; r[6] = -1;
  }
  __syncthreads();
  const unsigned ntiles = (n + BOX_TILE - 1) / BOX_TILE;
  const unsigned t0 = blockIdx.x * tiles_per_block;
  const unsigned t1 = t0 + tiles_per_block < ntiles ? t0 + tiles_per_block : ntiles;
  for (unsigned t = t0; t < t1; ++t) {
    const unsigned base = t * BOX_TILE;
    const unsigned v0 = base + tid * BOX_VEC;
    if (aligned && v0 + BOX_VEC <= n) {
      *reinterpret_cast<uint4*>(s_vox + tid * BOX_VEC) = *reinterpret_cast<const uint4*>(lab + v0);
    } else {
      for (int j = 0; j < BOX_VEC; ++j) s_vox[tid * BOX_VEC + j] = v0 + j < n ? lab[v0 + j] : (uint16_t)0;
    }
    __syncthreads();
    const unsigned wb = base + wave * BOX_WAVE;
    if (wb < n) {   // (the same for the whole wavefront)
      const unsigned rowb = wb / (unsigned)Y, yb = wb - rowb * (unsigned)Y;
      for (int s = 0; s < BOX_WAVE / 64; ++s) {
        const unsigned off = s * 64 + lane;
        const bool valid = wb + off < n;
        const int v = s_vox[wave * BOX_WAVE + off];
        const unsigned yl = yb + off;                                              // < Y + 512
        const unsigned q = Y >= BOX_WAVE ? (yl >= (unsigned)Y ? 1u : 0u) : yl / (unsigned)Y;   // rows past the wavefront's first
        const unsigned y = yl - q * (unsigned)Y;
        const int prev = __shfl_up(v, 1);
        const bool head = valid && (lane == 0 || v != prev || y == 0);
        const unsigned long long heads = __ballot(head);
        const unsigned long long valids = __ballot(valid);
        if (head && v > 0 && v <= L) {
          const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
          const int len = above ? __ffsll((long long)above) : __popcll(valids) - lane;   // valid lanes are the first ones
          const unsigned row = rowb + q;
          const int z = (int)(row / (unsigned)X), x = (int)(row - (unsigned)z * (unsigned)X);
          const int y0 = (int)y, y1 = (int)y + len - 1;                              // a run never leaves its row
          int slot = -1;
          unsigned h = ((unsigned)v * 0x9E3779B1u) >> (32 - BOX_SLOT_BITS);
          for (int p = 0; p < BOX_PROBES; ++p) {
            const int k = atomicCAS(&s_key[h], 0, v);
            if (k == 0 || k == v) { slot = (int)h; break; }
            h = (h + 1) & (BOX_SLOTS - 1);
          }
          if (slot >= 0) {
            int* r = s_val + slot * ROW;
            atomicAdd(r, len);
            atomicMin(r + 1, z); atomicMax(r + 2, z);
            atomicMin(r + 3, x); atomicMax(r + 4, x);
            atomicMin(r + 5, y0); atomicMax(r + 6, y1);
          } else {
            global_row_update(table + (size_t)v * ROW, len, z, z, x, x, y0, y1);
          }
        }
      }
    }
    __syncthreads();   // s_vox is staged again
  }
  for (int i = tid; i < BOX_SLOTS; i += BOX_THREADS) {
    const int k = s_key[i];
    if (k == 0) continue;
    const int* r = s_val + i * ROW;
    if (r[0] > 0) global_row_update(table + (size_t)k * ROW, r[0], r[1], r[2], r[3], r[4], r[5], r[6]);
  }
}

// ---- cubes around spots ------------------------------------------------------------------------------------------------
constexpr int VOTE_BINS = 2048;   // labels counted per pass; 32 such ranges cover 1..65535

__device__ inline void spot_centre(const double* __restrict__ centres, int i, int* cz, int* cx, int* cy) {
  *cz = round_centre(centres[3 * (size_t)i]);
  *cx = round_centre(centres[3 * (size_t)i + 1]);
  *cy = round_centre(centres[3 * (size_t)i + 2]);
}

// One wavefront per spot.  target != nullptr: out = 1 when the cube holds target[spot], else -1.  Otherwise the vote: the
// cube's labels are kept in LDS and counted exactly, one range of VOTE_BINS consecutive labels per pass (a counter per
// label, so a cube of (2r+1)^3 different labels is counted like any other); only ranges that occur in the cube get a
// pass.  The winner is the largest count, the smallest label among equal counts — where np.unique + np.argmax land —
// or -1 for a cube without a positive label.
__global__ __launch_bounds__(64) void cube_labels_k(const uint16_t* __restrict__ lab, int Z, int X, int Y,
                                                     const double* __restrict__ centres, int r, const int* __restrict__ target,
                                                     int* __restrict__ out) {
  __shared__ uint16_t s_cube[MAX_CUBE + 3];
  __shared__ unsigned s_cnt[VOTE_BINS];
  const int i = blockIdx.x, lane = threadIdx.x;
  const int w = 2 * r + 1, w3 = w * w * w;
  int cz, cx, cy;
  spot_centre(centres, i, &cz, &cx, &cy);
  if (target) {
    const int t = target[i];
    bool hit = false;
    for (int k = lane; k < w3; k += 64) hit = hit || (int)lab[cube_voxel(cz, cx, cy, k, r, Z, X, Y)] == t;
    const unsigned long long any = __ballot(hit);
    if (lane == 0) out[i] = any ? 1 : -1;
    return;
  }
  unsigned ranges = 0;   // bit p: a label of p * VOTE_BINS + 1 .. (p + 1) * VOTE_BINS occurs
  for (int k = lane; k < w3; k += 64) {
    const unsigned v = lab[cube_voxel(cz, cx, cy, k, r, Z, X, Y)];
    s_cube[k] = (uint16_t)v;
    if (v) ranges |= 1u << ((v - 1) / VOTE_BINS);
  }
  for (int o = 32; o; o >>= 1) ranges |= (unsigned)__shfl_xor((int)ranges, o);
  __syncthreads();
  int best_lab = -1;
  unsigned best_cnt = 0;
  while (ranges) {   // (the same for every lane) ascending ranges
    const unsigned first = (unsigned)(__ffs((int)ranges) - 1) * VOTE_BINS + 1;
    ranges &= ranges - 1;
    for (int j = lane; j < VOTE_BINS; j += 64) s_cnt[j] = 0;
    __syncthreads();
    for (int k = lane; k < w3; k += 64) {
      const unsigned d = (unsigned)s_cube[k] - first;   // background wraps to a large number
      if (d < (unsigned)VOTE_BINS) atomicAdd(&s_cnt[d], 1u);
    }
    __syncthreads();
    unsigned c = 0;
    int l = -1;
    for (int j = lane; j < VOTE_BINS; j += 64) {   // ascending labels: the first of equal counts stays
      const unsigned cc = s_cnt[j];
      if (cc > c) { c = cc; l = (int)first + j; }
    }
    for (int o = 32; o; o >>= 1) {
      const unsigned oc = (unsigned)__shfl_xor((int)c, o);
      const int ol = __shfl_xor(l, o);
      if (oc > c || (oc == c && oc > 0 && ol < l)) { c = oc; l = ol; }
    }
    if (c > best_cnt) { best_cnt = c; best_lab = l; }
    __syncthreads();
  }
  if (lane == 0) out[i] = best_lab;
}

// One wavefront per spot: np.max over the cube, NaN when the cube holds one
template <class T>
__global__ __launch_bounds__(64) void cube_max_k(const T* __restrict__ im, int Z, int X, int Y, const double* __restrict__ centres,
                                                  int r, T* __restrict__ out) {
  const int i = blockIdx.x, lane = threadIdx.x;
  const int w = 2 * r + 1, w3 = w * w * w;
  int cz, cx, cy;
  spot_centre(centres, i, &cz, &cx, &cy);
  T m = im[cube_voxel(cz, cx, cy, 0, r, Z, X, Y)];
  bool nan = m != m;
  for (int k = lane; k < w3; k += 64) {
    const T v = im[cube_voxel(cz, cx, cy, k, r, Z, X, Y)];
    if (v != v) nan = true;
    else if (!(m >= v)) m = v;   // (also replaces a NaN first value)
  }
  for (int o = 32; o; o >>= 1) {
    T om;
    if constexpr (sizeof(T) == 4) om = __shfl_xor(m, o);
    else om = (T)__shfl_xor((int)m, o);
    if (!(m >= om) && om == om) m = om;
  }
  const unsigned long long anynan = __ballot(nan);
  if (lane == 0) {
    if constexpr (sizeof(T) == 4) out[i] = anynan ? __builtin_nanf("") : m;
    else out[i] = m;
  }
}

// the (N, (2r+1)^3) matrix: one workgroup per spot, consecutive threads write consecutive columns
template <class T>
__global__ __launch_bounds__(256) void cube_gather_k(const T* __restrict__ im, int Z, int X, int Y, const double* __restrict__ centres,
                                                      int r, T* __restrict__ out) {
  const int i = blockIdx.x;
  const int w = 2 * r + 1, w3 = w * w * w;
  int cz, cx, cy;
  spot_centre(centres, i, &cz, &cx, &cy);
  T* row = out + (size_t)i * w3;
  for (int k = threadIdx.x; k < w3; k += 256) row[k] = im[cube_voxel(cz, cx, cy, k, r, Z, X, Y)];
}

int check_cube_args(const ia3_stack* im, const double* centres, int n, int radius, const void* out) {
  if (!im || !im->d) return set_error(IA3_EINVAL, "null stack");
  if (im->dtype != IA3_U16 && im->dtype != IA3_F32) return set_error(IA3_EINVAL, "unsupported dtype code %d", im->dtype);
  if (n < 0) return set_error(IA3_EINVAL, "negative spot count");
  if (radius < 0 || radius > MAX_RADIUS) return set_error(IA3_EINVAL, "search radius %d: 0 to %d", radius, MAX_RADIUS);
  if (im->Z < 1 || im->X < 1 || im->Y < 1) return set_error(IA3_EINVAL, "empty stack");
  if (n > 0 && (!centres || !out)) return set_error(IA3_EINVAL, "null argument");
  return IA3_OK;
}

constexpr int SPOTS_PER_LAUNCH = 1 << 20;

// per spot one value of B bytes: centres up, kernel, results down, SPOTS_PER_LAUNCH spots at a time
template <class Launch>
int per_spot_chunks(const double* centres, const int* target, int n, size_t out_bytes, void* out, const char* name, Launch launch) {
  hipStream_t st = stream();
  const int per = n < SPOTS_PER_LAUNCH ? n : SPOTS_PER_LAUNCH;
  Scratch cen((size_t)per * 3 * sizeof(double)), res((size_t)per * out_bytes), tar(target ? (size_t)per * sizeof(int) : 16);
  if (!cen.p || !res.p || !tar.p) return set_error(IA3_ENOMEM, "scratch for %d spots", per);
  for (int first = 0; first < n; first += per) {
    const int m = n - first < per ? n - first : per;
    IA3_HIP(hipMemcpyAsync(cen.p, centres + 3 * (size_t)first, (size_t)m * 3 * sizeof(double), hipMemcpyHostToDevice, st));
    if (target) IA3_HIP(hipMemcpyAsync(tar.p, target + first, (size_t)m * sizeof(int), hipMemcpyHostToDevice, st));
    {
      ProfScope ps(name);
      launch(m, cen.as<double>(), target ? tar.as<int>() : (int*)nullptr, res.p, st);
      IA3_KCHECK();
    }
    IA3_HIP(hipMemcpyAsync((char*)out + (size_t)first * out_bytes, res.p, (size_t)m * out_bytes, hipMemcpyDeviceToHost, st));
    IA3_HIP(hipStreamSynchronize(st));
  }
  return IA3_OK;
}

}  // namespace

extern "C" {

int ia3_label_boxes_dev(const ia3_stack* labels, int max_label, int* out7) {
  int rc = ensure_init(); if (rc) return rc;
  if (!labels || !labels->d || !out7) return set_error(IA3_EINVAL, "null argument");
  if (labels->dtype != IA3_U16) return set_error(IA3_EINVAL, "a label stack is uint16 (dtype code %d given)", labels->dtype);
  if (max_label < 1 || max_label > 65535) return set_error(IA3_EINVAL, "max_label %d: 1 to 65535", max_label);
  if (labels->Z < 1 || labels->X < 1 || labels->Y < 1) return set_error(IA3_EINVAL, "empty stack");
  const size_t nvox = (size_t)labels->Z * labels->X * labels->Y;
  if (nvox > (size_t)INT_MAX) return set_error(IA3_EUNSUPPORTED, "label stacks of up to 2^31 - 1 voxels are built (int32 counts)");
  hipStream_t st = stream();
  const int rows = max_label + 1;
  Scratch tab((size_t)rows * ROW * sizeof(int));
  if (!tab.p) return set_error(IA3_ENOMEM, "label table");
  const unsigned n = (unsigned)nvox;
  const unsigned ntiles = (n + BOX_TILE - 1) / BOX_TILE;
  unsigned blocks = (unsigned)num_cus() * 8u;
  if (blocks < 1) blocks = 1;
  if (blocks > ntiles) blocks = ntiles;
  const unsigned per = (ntiles + blocks - 1) / blocks;
  blocks = (ntiles + per - 1) / per;
  {
    ProfScope ps("label_boxes");
    hipLaunchKernelGGL(label_table_init_k, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, tab.as<int>(), rows);
    IA3_KCHECK();
    hipLaunchKernelGGL(label_boxes_k, dim3(blocks), dim3(BOX_THREADS), 0, st, (const uint16_t*)labels->d, n, labels->X, labels->Y,
                       max_label, ((uintptr_t)labels->d & 15) == 0 ? 1 : 0, per, tab.as<int>());
    IA3_KCHECK();
    hipLaunchKernelGGL(label_table_finish_k, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, tab.as<int>(), rows);
    IA3_KCHECK();
  }
  IA3_HIP(hipMemcpyAsync(out7, tab.p, (size_t)rows * ROW * sizeof(int), hipMemcpyDeviceToHost, st));
  IA3_HIP(hipStreamSynchronize(st));
  return IA3_OK;
}

int ia3_cube_labels_dev(const ia3_stack* labels, const double* centers_zxy, int n, int radius, const int* target, int* out) {
  int rc = ensure_init(); if (rc) return rc;
  rc = check_cube_args(labels, centers_zxy, n, radius, out); if (rc) return rc;
  if (labels->dtype != IA3_U16) return set_error(IA3_EINVAL, "a label stack is uint16 (dtype code %d given)", labels->dtype);
  if (n == 0) return IA3_OK;
  const ia3_stack* s = labels;
  return per_spot_chunks(centers_zxy, target, n, sizeof(int), out, target ? "cube_contains" : "cube_vote",
                         [=](int m, const double* cen, const int* tar, void* res, hipStream_t st) {
                           hipLaunchKernelGGL(cube_labels_k, dim3((unsigned)m), dim3(64), 0, st, (const uint16_t*)s->d, s->Z, s->X,
                                              s->Y, cen, radius, tar, (int*)res);
                         });
}

int ia3_cube_max_dev(const ia3_stack* im, const double* centers_zxy, int n, int radius, void* out) {
  int rc = ensure_init(); if (rc) return rc;
  rc = check_cube_args(im, centers_zxy, n, radius, out); if (rc) return rc;
  if (n == 0) return IA3_OK;
  const ia3_stack* s = im;
  return per_spot_chunks(centers_zxy, nullptr, n, esize(s->dtype), out, "cube_max",
                         [=](int m, const double* cen, const int*, void* res, hipStream_t st) {
                           if (s->dtype == IA3_F32)
                             hipLaunchKernelGGL((cube_max_k<float>), dim3((unsigned)m), dim3(64), 0, st, (const float*)s->d, s->Z, s->X,
                                                s->Y, cen, radius, (float*)res);
                           else
                             hipLaunchKernelGGL((cube_max_k<uint16_t>), dim3((unsigned)m), dim3(64), 0, st, (const uint16_t*)s->d, s->Z,
                                                s->X, s->Y, cen, radius, (uint16_t*)res);
                         });
}

int ia3_cube_gather_dev(const ia3_stack* im, const double* centers_zxy, int n, int radius, void* out) {
  int rc = ensure_init(); if (rc) return rc;
  rc = check_cube_args(im, centers_zxy, n, radius, out); if (rc) return rc;
  if (n == 0) return IA3_OK;
  const int w = 2 * radius + 1;
  const size_t row_bytes = (size_t)w * w * w * esize(im->dtype);
  // rows of at most 256 MB per launch
  hipStream_t st = stream();
  size_t fit = ((size_t)256 << 20) / row_bytes;
  if (fit < 1) fit = 1;
  const int per = fit < (size_t)n ? (int)fit : n;
  Scratch cen((size_t)per * 3 * sizeof(double)), res((size_t)per * row_bytes);
  if (!cen.p || !res.p) return set_error(IA3_ENOMEM, "scratch for %d cubes", per);
  for (int first = 0; first < n; first += per) {
    const int m = n - first < per ? n - first : per;
    IA3_HIP(hipMemcpyAsync(cen.p, centers_zxy + 3 * (size_t)first, (size_t)m * 3 * sizeof(double), hipMemcpyHostToDevice, st));
    {
      ProfScope ps("cube_gather");
      if (im->dtype == IA3_F32)
        hipLaunchKernelGGL((cube_gather_k<float>), dim3((unsigned)m), dim3(256), 0, st, (const float*)im->d, im->Z, im->X, im->Y,
                           cen.as<double>(), radius, res.as<float>());
      else
        hipLaunchKernelGGL((cube_gather_k<uint16_t>), dim3((unsigned)m), dim3(256), 0, st, (const uint16_t*)im->d, im->Z, im->X,
                           im->Y, cen.as<double>(), radius, res.as<uint16_t>());
      IA3_KCHECK();
    }
    IA3_HIP(hipMemcpyAsync((char*)out + (size_t)first * row_bytes, res.p, (size_t)m * row_bytes, hipMemcpyDeviceToHost, st));
    IA3_HIP(hipStreamSynchronize(st));
  }
  return IA3_OK;
}

}  // extern "C"
