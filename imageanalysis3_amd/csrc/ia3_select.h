// Exact order statistics of resident values by a segmented radix select (8 key bits per pass; uint16, float32 and float64
// keys), and the medians NumPy makes of them.  Shared by morph.hip (plane medians, the seed percentile) and chromim.hip
// (np.median of a whole stack).  Everything sits in an unnamed namespace: each translation unit has its own kernels.
#pragma once
#include "ia3_rt.h"
#include <math.h>
#include <string.h>
#include <vector>

namespace {
using namespace ia3rt;

typedef unsigned long long u64;

// ---- order-preserving keys ---------------------------------------------------------------------------------------------------
// NaNs of either sign order last, as np.sort puts them
template <class T> struct KeyOf;
template <> struct KeyOf<uint16_t> {
  static constexpr int BITS = 16;
  static __host__ __device__ inline u64 key(uint16_t v) { return v; }
};
template <> struct KeyOf<float> {
  static constexpr int BITS = 32;
  static __host__ __device__ inline u64 key(float v) {
    if (v != v) return 0xFFFFFFFFull;
    uint32_t b;
    memcpy(&b, &v, 4);
    return b & 0x80000000u ? (uint32_t)~b : (b | 0x80000000u);
  }
};
template <> struct KeyOf<double> {
  static constexpr int BITS = 64;
  static __host__ __device__ inline u64 key(double v) {
    if (v != v) return ~0ull;
    u64 b;
    memcpy(&b, &v, 8);
    return b >> 63 ? ~b : (b | (1ull << 63));
  }
};
float key_to_f32(u64 k) {
  uint32_t b = (uint32_t)k;
  b = b & 0x80000000u ? (b & 0x7FFFFFFFu) : ~b;
  float v;
  memcpy(&v, &b, 4);
  return v;
}
double key_to_f64(u64 k) {
  k = k >> 63 ? (k & ~(1ull << 63)) : ~k;
  double v;
  memcpy(&v, &k, 8);
  return v;
}

// ---- segmented radix select: two ranks in each of S equally long segments ---------------------------------------------------
struct SelSeg {
  u64 k[2];        // rank still to find among the values that share prefix[r]
  u64 prefix[2];   // key bits decided so far (high bits)
  unsigned nan;    // the segment holds a NaN
  unsigned pad;
};
constexpr int NB = 256;

__device__ __forceinline__ bool same_prefix(const SelSeg& s, int pass, int shift) {
  return pass == 0 || (s.prefix[0] >> (shift + 8)) == (s.prefix[1] >> (shift + 8));
}

// histogram of digit `pass` of the values of segment blockIdx.y whose higher digits equal a rank's prefix; the two ranks
// share one histogram while their prefixes agree.  hist: S x 2 x NB, zero before the launch.
template <class T>
__global__ __launch_bounds__(256) void seg_hist_k(const T* __restrict__ v, size_t seglen, int pass, SelSeg* __restrict__ st,
                                                  unsigned* __restrict__ hist) {
  __shared__ unsigned h[2 * NB];
  const int seg = blockIdx.y;
  const int shift = KeyOf<T>::BITS - 8 * (pass + 1);
  const SelSeg s = st[seg];
  const bool same = same_prefix(s, pass, shift);
  const u64 p0 = pass == 0 ? 0 : s.prefix[0] >> (shift + 8), p1 = pass == 0 ? 0 : s.prefix[1] >> (shift + 8);
  for (int i = threadIdx.x; i < 2 * NB; i += 256) h[i] = 0;
  __syncthreads();
  const T* p = v + (size_t)seg * seglen;
  bool nan = false;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < seglen; i += (size_t)gridDim.x * 256) {
    const T e = p[i];
    if (pass == 0 && e != e) nan = true;
    const u64 key = KeyOf<T>::key(e);
    const unsigned d = (unsigned)(key >> shift) & (NB - 1);
    const u64 hi = pass == 0 ? 0 : key >> (shift + 8);
    if (hi == p0) atomicAdd(&h[d], 1u);
    if (!same && hi == p1) atomicAdd(&h[NB + d], 1u);
  }
  if (nan) atomicOr(&st[seg].nan, 1u);
  __syncthreads();
  unsigned* out = hist + (size_t)seg * 2 * NB;
  for (int i = threadIdx.x; i < 2 * NB; i += 256)
    if (h[i]) atomicAdd(&out[i], h[i]);
}

// one thread per segment: each rank moves into the bucket that holds it
__global__ void seg_pick_k(SelSeg* __restrict__ st, const unsigned* __restrict__ hist, int S, int pass, int bits) {
  const int seg = blockIdx.x * blockDim.x + threadIdx.x;
  if (seg >= S) return;
  const int shift = bits - 8 * (pass + 1);
  SelSeg s = st[seg];
  const bool same = same_prefix(s, pass, shift);
  for (int r = 0; r < 2; ++r) {
    const unsigned* h = hist + ((size_t)seg * 2 + (r == 1 && !same ? 1 : 0)) * NB;
    u64 k = s.k[r], cum = 0;
    int b = 0;
    for (; b < NB; ++b) {
      const u64 c = h[b];
      if (cum + c > k) break;
      cum += c;
    }
    if (b >= NB) b = NB - 1;
    st[seg].prefix[r] = s.prefix[r] | ((u64)b << shift);
    st[seg].k[r] = k - cum;
  }
}

// keys of the order statistics k0 <= k1 of every segment (host: 2 per segment) and the NaN flags
template <class T>
int seg_select(const T* dev, int S, size_t seglen, u64 k0, u64 k1, std::vector<u64>& keys, std::vector<unsigned>& nan) {
  hipStream_t st = stream();
  std::vector<SelSeg> h((size_t)S);
  for (auto& s : h) { s.k[0] = k0; s.k[1] = k1; s.prefix[0] = s.prefix[1] = 0; s.nan = 0; s.pad = 0; }
  const size_t hist_bytes = (size_t)S * 2 * NB * sizeof(unsigned);
  Scratch dst((size_t)S * sizeof(SelSeg)), dh(hist_bytes);
  if (!dst.p || !dh.p) return set_error(IA3_ENOMEM, "scratch of the order statistics");
  IA3_HIP(hipMemcpyAsync(dst.p, h.data(), (size_t)S * sizeof(SelSeg), hipMemcpyHostToDevice, st));
  IA3_HIP(hipStreamSynchronize(st));   // h is pageable
  const size_t per_block = 256 * 32;
  size_t want = (seglen + per_block - 1) / per_block;
  size_t gmax = (size_t)num_cus() * 8 / (size_t)S;
  if (gmax < 1) gmax = 1;
  if (want > gmax) want = gmax;
  if (want < 1) want = 1;
  const int passes = KeyOf<T>::BITS / 8;
  {
    ProfScope ps("morph_select");
    for (int pass = 0; pass < passes; ++pass) {
      IA3_HIP(hipMemsetAsync(dh.p, 0, hist_bytes, st));
      hipLaunchKernelGGL((seg_hist_k<T>), dim3((unsigned)want, (unsigned)S), dim3(256), 0, st, dev, seglen, pass, dst.as<SelSeg>(),
                         dh.as<unsigned>());
      hipLaunchKernelGGL(seg_pick_k, dim3((unsigned)((S + 63) / 64)), dim3(64), 0, st, dst.as<SelSeg>(), (const unsigned*)dh.p, S,
                         pass, KeyOf<T>::BITS);
    }
    IA3_KCHECK();
  }
  IA3_HIP(hipMemcpyAsync(h.data(), dst.p, (size_t)S * sizeof(SelSeg), hipMemcpyDeviceToHost, st));
  IA3_HIP(hipStreamSynchronize(st));
  keys.resize((size_t)S * 2);
  nan.resize((size_t)S);
  for (int i = 0; i < S; ++i) { keys[2 * i] = h[i].prefix[0]; keys[2 * i + 1] = h[i].prefix[1]; nan[i] = h[i].nan; }
  return IA3_OK;
}

// np.median of each of S equally long segments, widened to float64.  kind: IA3_U16 (float64 mean of the two middle values
// for an even count), IA3_F32 (the two middle values added and halved in float32, as np.mean of two float32 does) or
// IA3_SEL_F64 (added and halved in float64).  NaN for a segment that holds one.
constexpr int IA3_SEL_F64 = 2;
int segment_medians(const void* d, int kind, int S, size_t seglen, std::vector<double>& med64) {
  const u64 k0 = (seglen - 1) / 2, k1 = seglen / 2;   // the middle value twice (odd count) or the two middle values
  std::vector<u64> keys;
  std::vector<unsigned> nan;
  int rc = kind == IA3_F32       ? seg_select<float>((const float*)d, S, seglen, k0, k1, keys, nan)
           : kind == IA3_SEL_F64 ? seg_select<double>((const double*)d, S, seglen, k0, k1, keys, nan)
                                 : seg_select<uint16_t>((const uint16_t*)d, S, seglen, k0, k1, keys, nan);
  if (rc) return rc;
  med64.resize((size_t)S);
  for (int z = 0; z < S; ++z) {
    if (kind == IA3_F32) {
      const float a = key_to_f32(keys[2 * z]), b = key_to_f32(keys[2 * z + 1]);
      volatile float sum = a + b;                       // np.mean of the two float32 values: added, then halved, in float32
      const float m = k0 == k1 ? a : sum / 2.0f;
      med64[z] = nan[z] ? (double)NAN : (double)m;
    } else if (kind == IA3_SEL_F64) {
      const double a = key_to_f64(keys[2 * z]), b = key_to_f64(keys[2 * z + 1]);
      volatile double sum = a + b;
      med64[z] = nan[z] ? (double)NAN : (k0 == k1 ? a : sum / 2.0);
    } else {
      const double a = (double)keys[2 * z], b = (double)keys[2 * z + 1];
      med64[z] = k0 == k1 ? a : (a + b) / 2.0;
    }
  }
  return IA3_OK;
}

}  // namespace
