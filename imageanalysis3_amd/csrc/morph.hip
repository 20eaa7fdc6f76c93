// Candidate chromosomes from a resident stack (reference: segmentation_tools/chromosome.py:264-361
// find_candidate_chromosomes) and the operators it is made of:
//   ia3_select.h              exact order statistics per plane or of a whole volume (radix select, 8 key bits per pass;
//                             uint16, float32 and float64 keys): np.median of every plane, scoreatpercentile of the seed
//   range_k                   maximum_filter - minimum_filter of lyr / np.median(lyr), mode 'nearest', in the image's
//                             arithmetic (uint16 and float64: float64, float32: float32)
//   mask_k                    seed > threshold with the edges cleared, one bit per voxel
//   morph_k                   binary erosion / dilation by ball(r) on bit rows (shifts, ANDs and ORs of words)
//   ccl_*_k                   6-connected labelling: union-find inside an LDS tile, atomicMin unions across tile faces,
//                             flatten, roots numbered in ascending flat index (scipy.ndimage.label's numbers), relabel
//   hole_*_k                  binary_fill_holes: the same labelling of the complement and a "touches a face" flag per root
//   label_sums_k              per label the voxel count and, per axis, the sum and number of the indices > 0
// Everything is order statistics, comparisons, bit work and integer sums (the two divisions of step 1 are correctly
// rounded), so results equal NumPy / SciPy bit for bit and are the same on every run.  The shared arithmetic is
// csrc/ia3_ccl.h, which tests/native/ccl_cpu.cpp builds for the host.
#include "ia3_rt.h"
#include "ia3_select.h"
#include "ia3_ccl.h"
#include <limits.h>
#include <math.h>
#include <string.h>
#include <vector>

using namespace ia3rt;

namespace {
using namespace ia3ccl;

// ---- range filter ------------------------------------------------------------------------------------------------------------
constexpr int RZ = 4, RX = 8, RY = 32;         // outputs of a block
constexpr int RH = 4;                          // largest halo (filter size 5)
constexpr int RLX = RX + RH, RLY = RY + RH;    // LDS tile pitches

__device__ __forceinline__ double quotient(uint16_t v, double m) { return (double)v / m; }   // IEEE division
__device__ __forceinline__ float quotient(float v, float m) { return __fdiv_rn(v, m); }
__device__ __forceinline__ double quotient(double v, double m) { return v / m; }             // IEEE division

// out = max - min over the s^3 window (offsets window_lo(s) .. window_hi(s), indices clamped) of im[z] / med[z].  The
// tile with its clamped halo is divided once while it is staged in LDS.
template <class T, class F>
__global__ __launch_bounds__(256) void range_k(const T* __restrict__ im, int Z, int X, int Y, const F* __restrict__ med, int s,
                                               F* __restrict__ out) {
  __shared__ F t[(RZ + RH) * RLX * RLY];
  const int z0 = blockIdx.z * RZ, x0 = blockIdx.y * RX, y0 = blockIdx.x * RY;
  const int lo = window_lo(s), ext = s - 1;
  const int nz = RZ + ext, nx = RX + ext, ny = RY + ext;
  for (int i = threadIdx.x; i < nz * nx * ny; i += 256) {
    const int ly = i % ny, lx = (i / ny) % nx, lz = i / (ny * nx);
    const int gz = clampi(z0 + lz + lo, 0, Z - 1), gx = clampi(x0 + lx + lo, 0, X - 1), gy = clampi(y0 + ly + lo, 0, Y - 1);
    t[(lz * RLX + lx) * RLY + ly] = quotient(im[((size_t)gz * X + gx) * Y + gy], med[gz]);
  }
  __syncthreads();
  const int ly = threadIdx.x & (RY - 1), lx = threadIdx.x / RY;
  const int gx = x0 + lx, gy = y0 + ly;
  if (gx >= X || gy >= Y) return;
  for (int lz = 0; lz < RZ; ++lz) {
    const int gz = z0 + lz;
    if (gz >= Z) break;
    F mn = t[(lz * RLX + lx) * RLY + ly], mx = mn;
    for (int a = 0; a < s; ++a)
      for (int b = 0; b < s; ++b)
        for (int c = 0; c < s; ++c) {
          const F v = t[((lz + a) * RLX + lx + b) * RLY + ly + c];
          mn = v < mn ? v : mn;
          mx = v > mx ? v : mx;
        }
    out[((size_t)gz * X + gx) * Y + gy] = mx - mn;
  }
}

// ---- masks: one wavefront per 64-bit word --------------------------------------------------------------------------------------
// seed > th in float64 (NumPy 2 compares a float32 array with a np.float64 scalar in float64), edges of width e cleared
template <class F>
__global__ __launch_bounds__(256) void mask_k(const F* __restrict__ seed, int Z, int X, int Y, int W, double th, int e,
                                              u64* __restrict__ bits, size_t nwords) {
  const size_t g = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= nwords) return;
  const int lane = threadIdx.x & 63;
  const size_t row = g / (size_t)W;
  const int w = (int)(g - row * (size_t)W), y = w * 64 + lane;
  const int z = (int)(row / (size_t)X), x = (int)(row - (size_t)z * X);
  bool on = false;
  if (y < Y && z >= e && z < Z - e && x >= e && x < X - e && y >= e && y < Y - e) on = (double)seed[row * (size_t)Y + y] > th;
  const u64 word = __ballot(on);
  if (lane == 0) bits[g] = word;
}

__global__ __launch_bounds__(256) void pack_k(const uint16_t* __restrict__ m, int X, int Y, int W, u64* __restrict__ bits,
                                              size_t nwords) {
  const size_t g = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= nwords) return;
  const int lane = threadIdx.x & 63;
  const size_t row = g / (size_t)W;
  const int y = (int)(g - row * (size_t)W) * 64 + lane;
  const u64 word = __ballot(y < Y && m[row * (size_t)Y + y] != 0);
  if (lane == 0) bits[g] = word;
}

__global__ __launch_bounds__(256) void unpack_k(const u64* __restrict__ bits, int Y, int W, uint16_t* __restrict__ m, size_t n) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= n) return;
  const size_t row = g / (size_t)Y;
  const int y = (int)(g - row * (size_t)Y);
  m[g] = (uint16_t)((bits[row * (size_t)W + (y >> 6)] >> (y & 63)) & 1);
}

// ---- erosion / dilation by ball(r) ---------------------------------------------------------------------------------------------
// one thread per word (ia3_ccl.h morph_word)
__global__ __launch_bounds__(256) void morph_k(const u64* __restrict__ in, int Z, int X, int Y, int W, int r, int dilate, int border,
                                               u64* __restrict__ out, size_t nwords) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= nwords) return;
  const size_t row = g / (size_t)W;
  const int w = (int)(g - row * (size_t)W);
  const int z = (int)(row / (size_t)X), x = (int)(row - (size_t)z * X);
  out[g] = morph_word((const uint64_t*)in, Z, X, Y, W, r, dilate, border, z, x, w);
}

// ---- connected components ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool bit_at(const u64* __restrict__ bits, int X, int W, int z, int x, int y, int invert) {
  return (((bits[((size_t)z * X + x) * (size_t)W + (y >> 6)] >> (y & 63)) & 1) != 0) != (invert != 0);
}

// 1. one TZ x TX x TY tile per block: union-find over the tile in LDS, then parent[voxel] = flat index of the tile-local
//    root (the smallest voxel of the piece of the component inside the tile), -1 for background
__global__ __launch_bounds__(256) void ccl_local_k(const u64* __restrict__ bits, int Z, int X, int Y, int W, int invert,
                                                   int* __restrict__ parent) {
  __shared__ int par[TILE];
  const int z0 = blockIdx.z * TZ, x0 = blockIdx.y * TX, y0 = blockIdx.x * TY;
  const int ly = threadIdx.x % TY, lx = threadIdx.x / TY;
  const int x = x0 + lx, y = y0 + ly;
  for (int lz = 0; lz < TZ; ++lz) {
    const int z = z0 + lz;
    const bool set = z < Z && x < X && y < Y && bit_at(bits, X, W, z, x, y, invert);
    par[tile_index(lz, lx, ly)] = set ? tile_index(lz, lx, ly) : -1;
  }
  __syncthreads();
  volatile int* vp = par;
  auto ld = [vp](int i) { return vp[i]; };
  auto amin = [](int i, int v) { return atomicMin(&par[i], v); };
  for (int lz = 0; lz < TZ; ++lz) {
    const int i = tile_index(lz, lx, ly);
    if (vp[i] < 0) continue;
    if (ly > 0 && vp[i - 1] >= 0) unite(ld, amin, i, i - 1);
    if (lx > 0 && vp[i - TY] >= 0) unite(ld, amin, i, i - TY);
    if (lz > 0 && vp[i - TX * TY] >= 0) unite(ld, amin, i, i - TX * TY);
  }
  __syncthreads();
  for (int lz = 0; lz < TZ; ++lz) {
    const int z = z0 + lz;
    if (z >= Z || x >= X || y >= Y) continue;
    const int i = tile_index(lz, lx, ly);
    int out = -1;
    if (vp[i] >= 0) {
      int rz, rx, ry;
      tile_coords(find_root(ld, i), &rz, &rx, &ry);
      out = (int)(((size_t)(z0 + rz) * X + (x0 + rx)) * Y + (y0 + ry));
    }
    parent[((size_t)z * X + x) * Y + y] = out;
  }
}

__device__ __forceinline__ int load_parent(const int* p, int i) {
  return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// 2. voxels on the low faces of a tile are joined to their set neighbour in the tile before: atomicMin onto the smaller
//    root, no waiting on anybody (ia3_ccl.h unite)
__global__ __launch_bounds__(256) void ccl_merge_k(int* parent, int Z, int X, int Y, unsigned n) {
  const unsigned g = blockIdx.x * 256u + threadIdx.x;
  if (g >= n) return;
  const int y = (int)(g % (unsigned)Y), x = (int)((g / (unsigned)Y) % (unsigned)X), z = (int)(g / ((unsigned)Y * (unsigned)X));
  const bool fy = y % TY == 0 && y > 0, fx = x % TX == 0 && x > 0, fz = z % TZ == 0 && z > 0;
  if (!(fy || fx || fz)) return;
  if (load_parent(parent, (int)g) < 0) return;
  auto ld = [parent](int i) { return load_parent(parent, i); };
  auto amin = [parent](int i, int v) { return atomicMin(parent + i, v); };
  if (fy && load_parent(parent, (int)g - 1) >= 0) unite(ld, amin, (int)g, (int)g - 1);
  if (fx && load_parent(parent, (int)g - Y) >= 0) unite(ld, amin, (int)g, (int)g - Y);
  if (fz && load_parent(parent, (int)g - X * Y) >= 0) unite(ld, amin, (int)g, (int)g - X * Y);
}

// 3. parent[voxel] = root.  In place: a concurrent reader sees the old parent or the root, both on the way to the root
__global__ __launch_bounds__(256) void ccl_flatten_k(int* parent, unsigned n) {
  const unsigned g = blockIdx.x * 256u + threadIdx.x;
  if (g >= n) return;
  if (load_parent(parent, (int)g) < 0) return;
  auto ld = [parent](int i) { return load_parent(parent, i); };
  const int r = find_root(ld, (int)g);
  __hip_atomic_store(parent + g, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// 4. roots numbered 1.. in ascending flat index: every thread takes NUM_PER consecutive voxels, every block NUM_CHUNK
constexpr int NUM_PER = 8;
constexpr int NUM_CHUNK = 256 * NUM_PER;

__device__ __forceinline__ int count_roots(const int* __restrict__ parent, unsigned n, unsigned first) {
  int c = 0;
  for (int j = 0; j < NUM_PER; ++j) {
    const unsigned g = first + j;
    if (g < n && parent[g] == (int)g) ++c;
  }
  return c;
}

__global__ __launch_bounds__(256) void ccl_count_k(const int* __restrict__ parent, unsigned n, int* __restrict__ block_count) {
  __shared__ int wsum[4];
  int c = count_roots(parent, n, blockIdx.x * (unsigned)NUM_CHUNK + threadIdx.x * NUM_PER);
  for (int o = 32; o; o >>= 1) c += __shfl_xor(c, o);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) block_count[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// exclusive sums of the block counts (one block; total[0] = number of roots)
__global__ __launch_bounds__(1024) void ccl_scan_k(int* __restrict__ block_count, int nblocks, int* __restrict__ total) {
  __shared__ int s[1024];
  __shared__ int carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (int base = 0; base < nblocks; base += 1024) {
    const int i = base + threadIdx.x;
    const int v = i < nblocks ? block_count[i] : 0;
    s[threadIdx.x] = v;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
      const int a = threadIdx.x >= o ? s[threadIdx.x - o] : 0;
      __syncthreads();
      s[threadIdx.x] += a;
      __syncthreads();
    }
    if (i < nblocks) block_count[i] = carry + s[threadIdx.x] - v;
    __syncthreads();
    if (threadIdx.x == 1023) carry += s[1023];
    __syncthreads();
  }
  if (threadIdx.x == 0) total[0] = carry;
}

__global__ __launch_bounds__(256) void ccl_number_k(const int* __restrict__ parent, unsigned n, const int* __restrict__ block_off,
                                                    int* __restrict__ lab) {
  __shared__ int s[256];
  const unsigned first = blockIdx.x * (unsigned)NUM_CHUNK + threadIdx.x * NUM_PER;
  const int c = count_roots(parent, n, first);
  s[threadIdx.x] = c;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const int a = threadIdx.x >= o ? s[threadIdx.x - o] : 0;
    __syncthreads();
    s[threadIdx.x] += a;
    __syncthreads();
  }
  int next = block_off[blockIdx.x] + s[threadIdx.x] - c + 1;
  for (int j = 0; j < NUM_PER; ++j) {
    const unsigned g = first + j;
    if (g < n && parent[g] == (int)g) lab[g] = next++;
  }
}

// 5. every other voxel takes its root's number (roots were written by ccl_number_k and are not written here)
__global__ __launch_bounds__(256) void ccl_relabel_k(const int* __restrict__ parent, unsigned n, int* lab) {
  const unsigned g = blockIdx.x * 256u + threadIdx.x;
  if (g >= n) return;
  const int p = parent[g];
  if (p == (int)g) return;
  lab[g] = p < 0 ? 0 : lab[p];
}

__global__ __launch_bounds__(256) void to_u16_k(const int* __restrict__ lab, unsigned n, uint16_t* __restrict__ out) {
  const unsigned g = blockIdx.x * 256u + threadIdx.x;
  if (g < n) out[g] = (uint16_t)lab[g];
}

// ---- fill holes ----------------------------------------------------------------------------------------------------------------
// flag[root] = 1 for every background component with a voxel on a face of the volume (all writers store the same value)
__global__ __launch_bounds__(256) void hole_faces_k(const int* __restrict__ parent, int Z, int X, int Y, unsigned n, int* flag) {
  const unsigned g = blockIdx.x * 256u + threadIdx.x;
  if (g >= n) return;
  const int p = parent[g];
  if (p < 0) return;
  const int y = (int)(g % (unsigned)Y), x = (int)((g / (unsigned)Y) % (unsigned)X), z = (int)(g / ((unsigned)Y * (unsigned)X));
  if (z == 0 || z == Z - 1 || x == 0 || x == X - 1 || y == 0 || y == Y - 1) flag[p] = 1;
}

__global__ __launch_bounds__(256) void hole_fill_k(const u64* __restrict__ in, const int* __restrict__ parent,
                                                   const int* __restrict__ flag, int Y, int W, u64* __restrict__ out, size_t nwords) {
  const size_t g = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= nwords) return;
  const int lane = threadIdx.x & 63;
  const size_t row = g / (size_t)W;
  const int y = (int)(g - row * (size_t)W) * 64 + lane;
  bool hole = false;
  if (y < Y) {
    const int p = parent[row * (size_t)Y + y];
    hole = p >= 0 && flag[p] == 0;
  }
  const u64 word = __ballot(hole);
  if (lane == 0) out[g] = in[g] | word;
}

// ---- per-label sums --------------------------------------------------------------------------------------------------------------
// 64 consecutive voxels per wavefront; labels are piecewise constant along a row, so only the first lane of a run (first
// lane, a change of label, a new row) adds, with the run's length: table[label] += ia3_ccl.h run_sums.  64-bit integer
// atomics: the sums do not depend on the order of arrival.
template <class LT>
__global__ __launch_bounds__(256) void label_sums_k(const LT* __restrict__ lab, unsigned n, int X, int Y, int L, u64* __restrict__ table) {
  const unsigned g = blockIdx.x * 256u + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool valid = g < n;
  const int v = valid ? (int)lab[g] : 0;
  const int y = valid ? (int)(g % (unsigned)Y) : 0;
  const int prev = __shfl_up(v, 1);
  const bool head = valid && (lane == 0 || v != prev || y == 0);
  const u64 heads = __ballot(head), valids = __ballot(valid);
  if (!(head && v > 0 && v <= L)) return;
  const u64 above = lane == 63 ? 0ull : heads >> (lane + 1);
  const int len = above ? __ffsll((long long)above) : __popcll(valids) - lane;
  const unsigned rowi = g / (unsigned)Y;
  const int z = (int)(rowi / (unsigned)X), x = (int)(rowi - (unsigned)z * (unsigned)X);
  u64 add[7];
  run_sums(z, x, y, len, add);
  u64* r = table + (size_t)v * 7;
#pragma unroll
  for (int k = 0; k < 7; ++k)
    if (add[k]) atomicAdd(r + k, add[k]);
}

// out = map[label] (labels above L become 0); in place is allowed
template <class LT>
__global__ __launch_bounds__(256) void label_map_k(const LT* lab, unsigned n, int L, const int* __restrict__ map, LT* out) {
  const unsigned g = blockIdx.x * 256u + threadIdx.x;
  if (g >= n) return;
  const int v = (int)lab[g];
  out[g] = (LT)(v > 0 && v <= L ? map[v] : 0);
}

template <class LT>
__global__ __launch_bounds__(256) void label_map_u16_k(const LT* __restrict__ lab, unsigned n, int L, const int* __restrict__ map,
                                                       uint16_t* __restrict__ out) {
  const unsigned g = blockIdx.x * 256u + threadIdx.x;
  if (g >= n) return;
  const int v = (int)lab[g];
  out[g] = (uint16_t)(v > 0 && v <= L ? map[v] : 0);
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
struct Dims {
  int Z, X, Y, W;
  unsigned n;
  size_t nwords;
};

int dims_of(const void* dev, int Z, int X, int Y, Dims& d) {
  if (!dev) return set_error(IA3_EINVAL, "null stack");
  if (Z < 1 || X < 1 || Y < 1) return set_error(IA3_EINVAL, "empty stack");
  const size_t nvox = (size_t)Z * X * Y;
  if (nvox > (size_t)INT_MAX) return set_error(IA3_EUNSUPPORTED, "stacks of up to 2^31 - 1 voxels are labelled (int32 parents and labels)");
  d.Z = Z; d.X = X; d.Y = Y; d.W = words_per_row(Y);
  d.n = (unsigned)nvox;
  d.nwords = (size_t)Z * X * d.W;
  return IA3_OK;
}
int dims_of(const ia3_stack* s, Dims& d) {
  if (!s) return set_error(IA3_EINVAL, "null stack");
  return dims_of(s->d, s->Z, s->X, s->Y, d);
}

int check_mask(const ia3_stack* m, Dims& d) {
  int rc = dims_of(m, d); if (rc) return rc;
  if (m->dtype != IA3_U16) return set_error(IA3_EINVAL, "a mask stack is uint16 (dtype code %d given)", m->dtype);
  return IA3_OK;
}

int same_shape_u16(const ia3_stack* out, const Dims& d, const char* what) {
  if (!out || !out->d) return set_error(IA3_EINVAL, "null %s", what);
  if (out->dtype != IA3_U16 || out->Z != d.Z || out->X != d.X || out->Y != d.Y)
    return set_error(IA3_EINVAL, "%s must be a uint16 stack of the input's shape", what);
  return IA3_OK;
}

inline unsigned blocks_of(size_t n, int per) { return (unsigned)((n + per - 1) / per); }

int pack_mask(const ia3_stack* m, const Dims& d, u64* bits) {
  hipLaunchKernelGGL(pack_k, dim3(blocks_of(d.nwords, 4)), dim3(256), 0, stream(), (const uint16_t*)m->d, d.X, d.Y, d.W, bits, d.nwords);
  IA3_KCHECK();
  return IA3_OK;
}
int unpack_mask(const u64* bits, const Dims& d, ia3_stack* out) {
  hipLaunchKernelGGL(unpack_k, dim3(blocks_of(d.n, 256)), dim3(256), 0, stream(), bits, d.Y, d.W, (uint16_t*)out->d, (size_t)d.n);
  IA3_KCHECK();
  return IA3_OK;
}

int morph(const u64* in, const Dims& d, int r, int dilate, int border, u64* out) {
  ProfScope ps(dilate ? "morph_dilate" : "morph_erode");
  hipLaunchKernelGGL(morph_k, dim3(blocks_of(d.nwords, 256)), dim3(256), 0, stream(), in, d.Z, d.X, d.Y, d.W, r, dilate, border, out,
                     d.nwords);
  IA3_KCHECK();
  return IA3_OK;
}

// parent[voxel] = smallest flat index of its 6-connected component among the set (invert: the clear) voxels, -1 elsewhere
int component_roots(const u64* bits, const Dims& d, int invert, int* parent) {
  hipStream_t st = stream();
  ProfScope ps("ccl_roots");
  hipLaunchKernelGGL(ccl_local_k, dim3(tiles(d.Y, TY), tiles(d.X, TX), tiles(d.Z, TZ)), dim3(256), 0, st, bits, d.Z, d.X, d.Y, d.W,
                     invert, parent);
  hipLaunchKernelGGL(ccl_merge_k, dim3(blocks_of(d.n, 256)), dim3(256), 0, st, parent, d.Z, d.X, d.Y, d.n);
  hipLaunchKernelGGL(ccl_flatten_k, dim3(blocks_of(d.n, 256)), dim3(256), 0, st, parent, d.n);
  IA3_KCHECK();
  return IA3_OK;
}

// lab = scipy.ndimage.label(mask)[0] (int32), *n_out = the number of components; parent: scratch of n ints
int label_bits(const u64* bits, const Dims& d, int* parent, int* lab, int* n_out) {
  hipStream_t st = stream();
  int rc = component_roots(bits, d, 0, parent); if (rc) return rc;
  const unsigned nb = blocks_of(d.n, NUM_CHUNK);
  Scratch cnt(((size_t)nb + 1) * sizeof(int));
  if (!cnt.p) return set_error(IA3_ENOMEM, "scratch of the label numbering");
  {
    ProfScope ps("ccl_number");
    hipLaunchKernelGGL(ccl_count_k, dim3(nb), dim3(256), 0, st, (const int*)parent, d.n, cnt.as<int>());
    hipLaunchKernelGGL(ccl_scan_k, dim3(1), dim3(1024), 0, st, cnt.as<int>(), (int)nb, cnt.as<int>() + nb);
    hipLaunchKernelGGL(ccl_number_k, dim3(nb), dim3(256), 0, st, (const int*)parent, d.n, (const int*)cnt.p, lab);
    hipLaunchKernelGGL(ccl_relabel_k, dim3(blocks_of(d.n, 256)), dim3(256), 0, st, (const int*)parent, d.n, lab);
    IA3_KCHECK();
  }
  IA3_HIP(hipMemcpyAsync(n_out, cnt.as<int>() + nb, sizeof(int), hipMemcpyDeviceToHost, st));
  IA3_HIP(hipStreamSynchronize(st));
  return IA3_OK;
}

int fill_holes(const u64* in, const Dims& d, u64* out) {
  hipStream_t st = stream();
  Scratch parent((size_t)d.n * sizeof(int)), flag((size_t)d.n * sizeof(int));
  if (!parent.p || !flag.p) return set_error(IA3_ENOMEM, "scratch of the hole filling");
  int rc = component_roots(in, d, 1, parent.as<int>()); if (rc) return rc;
  ProfScope ps("fill_holes");
  IA3_HIP(hipMemsetAsync(flag.p, 0, (size_t)d.n * sizeof(int), st));
  hipLaunchKernelGGL(hole_faces_k, dim3(blocks_of(d.n, 256)), dim3(256), 0, st, (const int*)parent.p, d.Z, d.X, d.Y, d.n, flag.as<int>());
  hipLaunchKernelGGL(hole_fill_k, dim3(blocks_of(d.nwords, 4)), dim3(256), 0, st, in, (const int*)parent.p, (const int*)flag.p, d.Y, d.W,
                     out, d.nwords);
  IA3_KCHECK();
  return IA3_OK;
}

// rows 0..L of [count, sum z, n(z > 0), sum x, n(x > 0), sum y, n(y > 0)] on the host
int label_sums(const void* lab, int bits, unsigned n, int X, int Y, int L, std::vector<u64>& table) {
  hipStream_t st = stream();
  const size_t bytes = ((size_t)L + 1) * 7 * sizeof(u64);
  Scratch tab(bytes);
  if (!tab.p) return set_error(IA3_ENOMEM, "label table");
  {
    ProfScope ps("label_sums");
    IA3_HIP(hipMemsetAsync(tab.p, 0, bytes, st));
    if (bits == 32) hipLaunchKernelGGL((label_sums_k<int>), dim3(blocks_of(n, 256)), dim3(256), 0, st, (const int*)lab, n, X, Y, L, tab.as<u64>());
    else hipLaunchKernelGGL((label_sums_k<uint16_t>), dim3(blocks_of(n, 256)), dim3(256), 0, st, (const uint16_t*)lab, n, X, Y, L, tab.as<u64>());
    IA3_KCHECK();
  }
  table.resize(((size_t)L + 1) * 7);
  IA3_HIP(hipMemcpyAsync(table.data(), tab.p, bytes, hipMemcpyDeviceToHost, st));
  IA3_HIP(hipStreamSynchronize(st));
  return IA3_OK;
}

// chromosome.py:4-10: per axis the mean of the indices > 0, integer sum over count in float64.  A label without such a
// voxel divides 0.0 by 0.0 at run time, as np.mean of an empty selection does: the same NaN, sign bit included.
void centre_of(const u64* row7, double* zxy) {
  for (int a = 0; a < 3; ++a) {
    volatile double sum = (double)row7[1 + 2 * a], cnt = (double)row7[2 + 2 * a];
    zxy[a] = sum / cnt;
  }
}

int check_labels(const void* lab, int bits, int Z, int X, int Y, int max_label, unsigned* n) {
  if (!lab) return set_error(IA3_EINVAL, "null label volume");
  if (bits != 16 && bits != 32) return set_error(IA3_EINVAL, "labels are 16 or 32 bits wide, got %d", bits);
  if (Z < 1 || X < 1 || Y < 1) return set_error(IA3_EINVAL, "empty stack");
  const size_t nvox = (size_t)Z * X * Y;
  if (nvox > (size_t)INT_MAX) return set_error(IA3_EUNSUPPORTED, "label volumes of up to 2^31 - 1 voxels are supported");
  if (max_label < 0 || (bits == 16 && max_label > 65535)) return set_error(IA3_EINVAL, "max_label %d out of range", max_label);
  *n = (unsigned)nvox;
  return IA3_OK;
}

int upload_map(const std::vector<int>& map, Scratch& dmap) {
  IA3_HIP(hipMemcpyAsync(dmap.p, map.data(), map.size() * sizeof(int), hipMemcpyHostToDevice, stream()));
  IA3_HIP(hipStreamSynchronize(stream()));
  return IA3_OK;
}

// seed image of chromosome.py:296-299 into `seed` (float32 for a float32 stack, float64 for a uint16 stack and for a
// float64 volume)
int range_image(const void* im, int kind, const Dims& d, const std::vector<double>& med64, int fs, void* seed) {
  hipStream_t st = stream();
  const bool f32 = kind == IA3_F32;
  Scratch dmed((size_t)d.Z * sizeof(double));
  if (!dmed.p) return set_error(IA3_ENOMEM, "plane medians");
  std::vector<float> med32;
  if (f32) {
    med32.resize((size_t)d.Z);
    for (int z = 0; z < d.Z; ++z) med32[z] = (float)med64[z];   // exact: the median was made in float32
    IA3_HIP(hipMemcpyAsync(dmed.p, med32.data(), (size_t)d.Z * sizeof(float), hipMemcpyHostToDevice, st));
  } else {
    IA3_HIP(hipMemcpyAsync(dmed.p, med64.data(), (size_t)d.Z * sizeof(double), hipMemcpyHostToDevice, st));
  }
  IA3_HIP(hipStreamSynchronize(st));
  ProfScope ps("morph_range");
  const dim3 grid(tiles(d.Y, RY), tiles(d.X, RX), tiles(d.Z, RZ));
  if (f32) hipLaunchKernelGGL((range_k<float, float>), grid, dim3(256), 0, st, (const float*)im, d.Z, d.X, d.Y, (const float*)dmed.p, fs, (float*)seed);
  else if (kind == IA3_SEL_F64) hipLaunchKernelGGL((range_k<double, double>), grid, dim3(256), 0, st, (const double*)im, d.Z, d.X, d.Y, (const double*)dmed.p, fs, (double*)seed);
  else hipLaunchKernelGGL((range_k<uint16_t, double>), grid, dim3(256), 0, st, (const uint16_t*)im, d.Z, d.X, d.Y, (const double*)dmed.p, fs, (double*)seed);
  IA3_KCHECK();
  return IA3_OK;
}

// scipy.stats.scoreatpercentile over all n values: the two neighbouring order statistics weighted in float64
template <class F>
int percentile_of(const F* seed, size_t n, double per, double* out) {
  long long i;
  double idx;
  percentile_index(per, (long long)n, &i, &idx);
  Select<false> sel(1);
  Scratch dv(2 * sizeof(F));
  if (!sel.ok() || !dv.p) return set_error(IA3_ENOMEM, "scratch of the order statistics");
  int rc;
  {
    ProfScope ps("morph_select");
    rc = sel.run(seed, n, SelRanks{{(u64)i, (u64)percentile_next(i, (long long)n)}, 2}); if (rc) return rc;
    rc = sel.values(dv.as<F>()); if (rc) return rc;
  }
  F v[2];
  rc = fetch(dv.as<F>(), 2, v); if (rc) return rc;
  *out = percentile_value(idx, i, (double)v[0], (double)v[1]);
  return IA3_OK;
}

int check_image(const ia3_stack* im, Dims& d) {
  int rc = dims_of(im, d); if (rc) return rc;
  if (im->dtype != IA3_U16 && im->dtype != IA3_F32) return set_error(IA3_EINVAL, "stack dtype must be uint16 or float32");
  return IA3_OK;
}

int check_seed_args(int filt_size, double per) {
  if (filt_size < 1 || filt_size > 5) return set_error(IA3_EUNSUPPORTED, "_filt_size %d: the range filter is built for sizes 1 to 5", filt_size);
  if (!(per >= 0 && per <= 100)) return set_error(IA3_EINVAL, "percentile must be in the range [0, 100]");
  return IA3_OK;
}

// steps 1-2 of find_candidate_chromosomes (chromosome.py:293-311): the thresholded, edge-cleared mask as bits
int seed_mask_bits(const void* im, int kind, const Dims& d, int filt_size, double per, u64* bits, double* threshold) {
  std::vector<double> med;
  // np.median of every plane as the reference's division sees it (chromosome.py:296), widened to float64
  int rc = host_medians("morph_select", im, kind, d.Z, (size_t)d.X * d.Y, med); if (rc) return rc;
  for (int z = 0; z < d.Z; ++z)
    if (!(med[z] != 0) || !isfinite(med[z]))
      return set_error(IA3_EINVAL, "plane %d has the median %g: the layer adjustment divides by it", z, med[z]);
  const bool f32 = kind == IA3_F32;
  Scratch seed((size_t)d.n * (f32 ? sizeof(float) : sizeof(double)));
  if (!seed.p) return set_error(IA3_ENOMEM, "seed image of %u voxels", d.n);
  rc = range_image(im, kind, d, med, filt_size, seed.p); if (rc) return rc;
  rc = f32 ? percentile_of<float>(seed.as<float>(), d.n, per, threshold) : percentile_of<double>(seed.as<double>(), d.n, per, threshold);
  if (rc) return rc;
  ProfScope ps("morph_mask");
  const int e = edge_width(filt_size);
  if (f32) hipLaunchKernelGGL((mask_k<float>), dim3(blocks_of(d.nwords, 4)), dim3(256), 0, stream(), (const float*)seed.p, d.Z, d.X, d.Y, d.W, *threshold, e, bits, d.nwords);
  else hipLaunchKernelGGL((mask_k<double>), dim3(blocks_of(d.nwords, 4)), dim3(256), 0, stream(), (const double*)seed.p, d.Z, d.X, d.Y, d.W, *threshold, e, bits, d.nwords);
  IA3_KCHECK();
  IA3_HIP(hipStreamSynchronize(stream()));   // `seed` goes back to the cache
  return IA3_OK;
}

// find_candidate_chromosomes (chromosome.py:264-361) of a resident uint16 / float32 stack or float64 volume
int candidate_chromosomes(const void* im, int kind, const Dims& d, const ia3_chrom_params* p, double* coords_zxy, int capacity,
                          int* n_out, double* threshold, ia3_stack* kept_labels) {
  if (!p || !n_out || !threshold) return set_error(IA3_EINVAL, "null argument");
  int rc = check_seed_args(p->filt_size, p->binary_per_th); if (rc) return rc;
  if (p->morphology_size != 1)
    return set_error(IA3_EUNSUPPORTED, "_morphology_size %d: the fused entry is built for ball(1), where a hole is a 6-connected background component; compose the operators for other sizes", p->morphology_size);
  if (capacity < 0 || (capacity > 0 && !coords_zxy)) return set_error(IA3_EINVAL, "bad coordinate table");
  if (kept_labels) { rc = same_shape_u16(kept_labels, d, "kept-label stack"); if (rc) return rc; }
  *n_out = 0;
  Scratch a(d.nwords * sizeof(u64)), b(d.nwords * sizeof(u64));
  if (!a.p || !b.p) return set_error(IA3_ENOMEM, "mask bits");
  u64 *A = a.as<u64>(), *B = b.as<u64>();
  rc = seed_mask_bits(im, kind, d, p->filt_size, p->binary_per_th, A, threshold); if (rc) return rc;
  // chromosome.py:317-319: opening by ball(1) (outside counts as clear for both halves), holes filled
  rc = morph(A, d, 1, 0, 0, B); if (rc) return rc;
  rc = morph(B, d, 1, 1, 0, A); if (rc) return rc;
  rc = fill_holes(A, d, B); if (rc) return rc;
  // :323-324: opening by ball(0) is the identity; closing by ball(1) (its border rule cannot matter here)
  rc = morph(B, d, 1, 1, 0, A); if (rc) return rc;
  rc = morph(A, d, 1, 0, 1, B); if (rc) return rc;
  // :325-337: label; the random walker returns fully labelled input as it is; small labels go
  Scratch parent((size_t)d.n * sizeof(int)), lab((size_t)d.n * sizeof(int));
  if (!parent.p || !lab.p) return set_error(IA3_ENOMEM, "scratch of the labelling");
  int n = 0;
  rc = label_bits(B, d, parent.as<int>(), lab.as<int>(), &n); if (rc) return rc;
  if (n > 65535) return set_error(IA3_EUNSUPPORTED, "%d components do not fit the reference's uint16 labels (it wraps silently)", n);
  std::vector<int> map((size_t)n + 1, 0);
  int kept = 0;
  std::vector<u64> table;
  if (n > 0) {
    rc = label_sums(lab.p, 32, d.n, d.X, d.Y, n, table); if (rc) return rc;
    for (int l = 1; l <= n; ++l)
      if ((long long)table[(size_t)l * 7] >= (long long)p->min_label_size) { map[l] = l; ++kept; }
  }
  if (kept_labels) {
    Scratch dmap(map.size() * sizeof(int));
    if (!dmap.p) return set_error(IA3_ENOMEM, "label map");
    rc = upload_map(map, dmap); if (rc) return rc;
    hipLaunchKernelGGL((label_map_u16_k<int>), dim3(blocks_of(d.n, 256)), dim3(256), 0, stream(), (const int*)lab.p, d.n, n, (const int*)dmap.p, (uint16_t*)kept_labels->d);
    IA3_KCHECK();
    IA3_HIP(hipStreamSynchronize(stream()));
  }
  *n_out = kept;
  if (kept > capacity) return set_error(IA3_ECAPACITY, "%d candidate chromosomes, room for %d", kept, capacity);
  int row = 0;
  for (int l = 1; l <= n; ++l)
    if (map[l]) centre_of(&table[(size_t)l * 7], coords_zxy + 3 * (size_t)row++);
  return IA3_OK;
}

}  // namespace

extern "C" {

int ia3_plane_medians_dev(const ia3_stack* s, double* out) {
  int rc = ensure_init(); if (rc) return rc;
  Dims d;
  rc = check_image(s, d); if (rc) return rc;
  if (!out) return set_error(IA3_EINVAL, "null output");
  std::vector<double> med;
  rc = host_medians("morph_select", s->d, s->dtype, d.Z, (size_t)d.X * d.Y, med); if (rc) return rc;
  memcpy(out, med.data(), (size_t)d.Z * sizeof(double));
  return IA3_OK;
}

int ia3_chrom_seed_mask_dev(const ia3_stack* im, int filt_size, double binary_per_th, ia3_stack* mask_out, double* threshold) {
  int rc = ensure_init(); if (rc) return rc;
  Dims d;
  rc = check_image(im, d); if (rc) return rc;
  rc = check_seed_args(filt_size, binary_per_th); if (rc) return rc;
  if (!threshold) return set_error(IA3_EINVAL, "null threshold");
  rc = same_shape_u16(mask_out, d, "mask"); if (rc) return rc;
  Scratch bits(d.nwords * sizeof(u64));
  if (!bits.p) return set_error(IA3_ENOMEM, "mask bits");
  rc = seed_mask_bits(im->d, im->dtype, d, filt_size, binary_per_th, bits.as<u64>(), threshold); if (rc) return rc;
  return unpack_mask(bits.as<u64>(), d, mask_out);
}

int ia3_binary_morph_dev(const ia3_stack* mask, int op, int radius, int border, ia3_stack* out) {
  int rc = ensure_init(); if (rc) return rc;
  Dims d;
  rc = check_mask(mask, d); if (rc) return rc;
  rc = same_shape_u16(out, d, "output"); if (rc) return rc;
  if (op < IA3_MORPH_ERODE || op > IA3_MORPH_CLOSE) return set_error(IA3_EINVAL, "unknown morphology operation %d", op);
  if (radius < 0 || radius > 2) return set_error(IA3_EUNSUPPORTED, "ball(%d): the bit-row operators are built for radius 0 to 2", radius);
  Scratch a(d.nwords * sizeof(u64)), b(d.nwords * sizeof(u64));
  if (!a.p || !b.p) return set_error(IA3_ENOMEM, "mask bits");
  rc = pack_mask(mask, d, a.as<u64>()); if (rc) return rc;
  if (op == IA3_MORPH_CLOSE) {   // dilation, then an erosion for which the outside counts as set
    rc = morph(a.as<u64>(), d, radius, 1, 0, b.as<u64>()); if (rc) return rc;
    rc = morph(b.as<u64>(), d, radius, 0, 1, a.as<u64>()); if (rc) return rc;
    return unpack_mask(a.as<u64>(), d, out);
  }
  rc = morph(a.as<u64>(), d, radius, op == IA3_MORPH_DILATE ? 1 : 0, border ? 1 : 0, b.as<u64>()); if (rc) return rc;
  return unpack_mask(b.as<u64>(), d, out);
}

int ia3_binary_fill_holes_dev(const ia3_stack* mask, ia3_stack* out) {
  int rc = ensure_init(); if (rc) return rc;
  Dims d;
  rc = check_mask(mask, d); if (rc) return rc;
  rc = same_shape_u16(out, d, "output"); if (rc) return rc;
  Scratch a(d.nwords * sizeof(u64)), b(d.nwords * sizeof(u64));
  if (!a.p || !b.p) return set_error(IA3_ENOMEM, "mask bits");
  rc = pack_mask(mask, d, a.as<u64>()); if (rc) return rc;
  rc = fill_holes(a.as<u64>(), d, b.as<u64>()); if (rc) return rc;
  return unpack_mask(b.as<u64>(), d, out);
}

int ia3_label_dev(const ia3_stack* mask, int* labels_dev, int* n_out, ia3_stack* labels16) {
  int rc = ensure_init(); if (rc) return rc;
  Dims d;
  rc = check_mask(mask, d); if (rc) return rc;
  if (!labels_dev || !n_out) return set_error(IA3_EINVAL, "null argument");
  if (labels16) { rc = same_shape_u16(labels16, d, "label stack"); if (rc) return rc; }
  Scratch bits(d.nwords * sizeof(u64)), parent((size_t)d.n * sizeof(int));
  if (!bits.p || !parent.p) return set_error(IA3_ENOMEM, "scratch of the labelling");
  rc = pack_mask(mask, d, bits.as<u64>()); if (rc) return rc;
  rc = label_bits(bits.as<u64>(), d, parent.as<int>(), labels_dev, n_out); if (rc) return rc;
  if (labels16) {
    if (*n_out > 65535) return set_error(IA3_EUNSUPPORTED, "%d components do not fit uint16 labels (the reference wraps silently)", *n_out);
    hipLaunchKernelGGL(to_u16_k, dim3(blocks_of(d.n, 256)), dim3(256), 0, stream(), (const int*)labels_dev, d.n, (uint16_t*)labels16->d);
    IA3_KCHECK();
  }
  return IA3_OK;
}

int ia3_label_centers_dev(const void* labels_dev, int label_bits_, int Z, int X, int Y, int max_label, double* centers_zxy,
                          long long* counts) {
  int rc = ensure_init(); if (rc) return rc;
  unsigned n;
  rc = check_labels(labels_dev, label_bits_, Z, X, Y, max_label, &n); if (rc) return rc;
  if (max_label == 0) return IA3_OK;
  if (!centers_zxy || !counts) return set_error(IA3_EINVAL, "null output");
  std::vector<u64> table;
  rc = label_sums(labels_dev, label_bits_, n, X, Y, max_label, table); if (rc) return rc;
  for (int l = 1; l <= max_label; ++l) {
    counts[l - 1] = (long long)table[(size_t)l * 7];
    centre_of(&table[(size_t)l * 7], centers_zxy + 3 * (size_t)(l - 1));
  }
  return IA3_OK;
}

int ia3_remove_small_labels_dev(const void* labels_dev, int label_bits_, int Z, int X, int Y, int max_label, long long min_size,
                                void* out_dev) {
  int rc = ensure_init(); if (rc) return rc;
  unsigned n;
  rc = check_labels(labels_dev, label_bits_, Z, X, Y, max_label, &n); if (rc) return rc;
  if (!out_dev) return set_error(IA3_EINVAL, "null output");
  std::vector<u64> table;
  rc = label_sums(labels_dev, label_bits_, n, X, Y, max_label, table); if (rc) return rc;
  std::vector<int> map((size_t)max_label + 1, 0);
  for (int l = 1; l <= max_label; ++l) map[l] = (long long)table[(size_t)l * 7] >= min_size ? l : 0;
  Scratch dmap(map.size() * sizeof(int));
  if (!dmap.p) return set_error(IA3_ENOMEM, "label map");
  rc = upload_map(map, dmap); if (rc) return rc;
  ProfScope ps("label_map");
  if (label_bits_ == 32) hipLaunchKernelGGL((label_map_k<int>), dim3(blocks_of(n, 256)), dim3(256), 0, stream(), (const int*)labels_dev, n, max_label, (const int*)dmap.p, (int*)out_dev);
  else hipLaunchKernelGGL((label_map_k<uint16_t>), dim3(blocks_of(n, 256)), dim3(256), 0, stream(), (const uint16_t*)labels_dev, n, max_label, (const int*)dmap.p, (uint16_t*)out_dev);
  IA3_KCHECK();
  IA3_HIP(hipStreamSynchronize(stream()));   // dmap goes back to the cache
  return IA3_OK;
}

int ia3_find_candidate_chromosomes_dev(const ia3_stack* im, const ia3_chrom_params* p, double* coords_zxy, int capacity, int* n_out,
                                       double* threshold, ia3_stack* kept_labels) {
  int rc = ensure_init(); if (rc) return rc;
  Dims d;
  rc = check_image(im, d); if (rc) return rc;
  return candidate_chromosomes(im->d, im->dtype, d, p, coords_zxy, capacity, n_out, threshold, kept_labels);
}

int ia3_find_candidate_chromosomes_f64_dev(const ia3_chrom_image* im, const ia3_chrom_params* p, double* coords_zxy, int capacity,
                                           int* n_out, double* threshold, ia3_stack* kept_labels) {
  int rc = ensure_init(); if (rc) return rc;
  if (!im) return set_error(IA3_EINVAL, "null chromosome image");
  Dims d;
  rc = dims_of(im->d, im->Z, im->X, im->Y, d); if (rc) return rc;
  return candidate_chromosomes(im->d, IA3_SEL_F64, d, p, coords_zxy, capacity, n_out, threshold, kept_labels);
}

}  // extern "C"
