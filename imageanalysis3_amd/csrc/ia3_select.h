// Exact order statistics of resident values by a most-significant-digit radix select, 8 key bits per
// pass: uint16 takes 2 passes, float32 4, float64 8.  The problems of one select are S consecutive, equally long segments
// of one array, each asked for the same list of up to MAXR ranks, and optionally the union of all segments with up to
// MAXU ranks of its own (the z-shift: every plane and the whole stack).  Used by corrections.hip, stats.hip, morph.hip and
// chromim.hip; everything sits in an unnamed namespace, so each translation unit has its own kernels.
//
// A pass makes, per problem, one histogram of the pass's digit for every distinct prefix its ranks have decided so far
// (the two ranks around a median or a percentile nearly always share theirs); then every rank picks the bin that holds
// it.  Blocks count into LDS with integer atomics and add their histograms to the global ones once: integer sums, so the
// result does not depend on the schedule.  Bins count in 32 bits (a stack holds < 2^32 voxels), ranks in 64.  The state
// is made, advanced and read on the device: nothing here waits for the stream but fetch().
#pragma once
#include "ia3_rt.h"
#include "ia3_order.h"
#include <math.h>
#include <type_traits>
#include <vector>

namespace {
using namespace ia3rt;
using namespace ia3ord;

constexpr int MAXR = 16;      // ranks of a segment
constexpr int MAXU = 8;       // ranks of the union
constexpr int NB = 256;       // bins of a pass
constexpr int IA3_SEL_F64 = 2;   // float64 values, beside IA3_U16 and IA3_F32

struct SelRanks {
  u64 k[MAXR];
  int n;
};
// the ranks a median needs: the middle one or two and, for floating-point values, the largest, whose key tells whether
// the problem holds a NaN (NaN keys are the largest there are)
template <class T>
SelRanks middle_ranks(u64 count) { return SelRanks{{mid_lo(count), mid_hi(count), count - 1}, std::is_floating_point<T>::value ? 3 : 2}; }

struct SelProb {          // one problem: a segment, or the union
  u64 k[MAXR];            // rank still to find among the values that share prefix[r]
  u64 prefix[MAXR];       // key bits decided so far (high bits); after the last pass the key of the order statistic
  u64 gprefix[MAXR];      // the distinct prefixes
  int grp[MAXR];          // rank -> index into gprefix
  int n, ngrp;
};

// problems 0 .. S-1 are the segments; problem S, if there is one, is the union
__global__ void sel_init_k(SelProb* st, int S, int nprob, SelRanks seg, SelRanks uni) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nprob) return;
  const SelRanks& r = q < S ? seg : uni;
  SelProb& p = st[q];
  for (int i = 0; i < MAXR; ++i) {
    p.k[i] = i < r.n ? r.k[i] : 0;
    p.prefix[i] = 0; p.gprefix[i] = 0; p.grp[i] = 0;
  }
  p.n = r.n; p.ngrp = 1;
}

// Histograms of digit `pass` of segment blockIdx.y: rows 0 .. ng-1 of the LDS table count for the segment's groups, rows
// ng .. ng+nu-1 for the union's.  16-byte loads over the aligned body of the segment; the elements before its first
// 16-byte boundary and after its last whole vector go one by one (block 0 of the segment).  hist: the pass's MAXR x NB
// bins per problem, zero before the launch.
template <class T, bool UNION>
__global__ __launch_bounds__(256) void sel_hist_k(const T* __restrict__ v, size_t seglen, int S, int pass,
                                                  const SelProb* __restrict__ st, unsigned* __restrict__ hist) {
  typedef typename KeyOf<T>::K K;
  constexpr int V = 16 / sizeof(T), MAXG = MAXR + (UNION ? MAXU : 0);
  __shared__ unsigned h[MAXG * NB];
  __shared__ K gp[MAXG];
  static_assert(sizeof(h) + sizeof(gp) <= 32768, "the segment's and the union's groups share 32 KB of LDS");
  const int seg = blockIdx.y;
  const int shift = KeyOf<T>::BITS - 8 * (pass + 1);
  const int ng = st[seg].ngrp, nu = UNION ? st[S].ngrp : 0, ngu = ng + nu;
  for (int i = threadIdx.x; i < ngu * NB; i += 256) h[i] = 0;
  if (pass > 0 && threadIdx.x < MAXG) {   // thread t < MAXR: the segment's group t, the others the union's; loaded whatever ng is
    const int t = threadIdx.x < MAXR ? threadIdx.x : threadIdx.x - MAXR;
    const u64 p = threadIdx.x < MAXR ? st[seg].gprefix[t] : st[S].gprefix[t];
    if (threadIdx.x < MAXR ? t < ng : t < nu) gp[threadIdx.x < MAXR ? t : ng + t] = (K)p >> (shift + 8);
  }
  __syncthreads();
  auto count = [&](T e) {
    const K key = KeyOf<T>::key(e);
    const unsigned d = (unsigned)(key >> shift) & (NB - 1);
    if (pass == 0) {   // every problem has one group, which takes everything: rows 0 and 1
      atomicAdd(&h[d], 1u);
      if (UNION) atomicAdd(&h[NB + d], 1u);
      return;
    }
    const K hi = key >> (shift + 8);
    for (int g = 0; g < ngu; ++g)
      if (hi == gp[g]) atomicAdd(&h[g * NB + d], 1u);
  };
  const T* p = v + (size_t)seg * seglen;
  size_t head = ((16 - ((uintptr_t)p & 15)) & 15) / sizeof(T);
  if (head > seglen) head = seglen;
  const size_t nvec = (seglen - head) / V, tail0 = head + nvec * V;
  if (blockIdx.x == 0) {
    for (size_t i = threadIdx.x; i < head; i += 256) count(p[i]);
    for (size_t i = tail0 + threadIdx.x; i < seglen; i += 256) count(p[i]);
  }
  const uint4* body = (const uint4*)(p + head);
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (size_t)gridDim.x * 256) {
    const uint4 q = body[i];
    T e[V];
    __builtin_memcpy(e, &q, 16);
#pragma unroll
    for (int j = 0; j < V; ++j) count(e[j]);
  }
  __syncthreads();
  unsigned* out = hist + (size_t)seg * MAXR * NB;
  for (int i = threadIdx.x; i < ngu * NB; i += 256) {
    if (!h[i]) continue;
    if (!UNION || i < ng * NB) atomicAdd(&out[i], h[i]);
    else atomicAdd(&hist[(size_t)S * MAXR * NB + (i - ng * NB)], h[i]);
  }
}

// one thread per (problem, rank) moves the rank into the bin that holds it; then each problem lists its groups again
__global__ __launch_bounds__(64) void sel_pick_k(SelProb* st, const unsigned* __restrict__ hist, int nprob, int shift) {
  const int q = blockIdx.x * (64 / MAXR) + threadIdx.x / MAXR, r = threadIdx.x % MAXR;
  if (q < nprob && r < st[q].n) {
    u64 k = st[q].k[r];
    const int b = pick_bin(hist + ((size_t)q * MAXR + st[q].grp[r]) * NB, NB, k);
    st[q].prefix[r] |= (u64)b << shift;
    st[q].k[r] = k;
  }
  __syncthreads();
  if (q < nprob && r == 0) st[q].ngrp = regroup(st[q].prefix, st[q].n, st[q].gprefix, st[q].grp);
}

// out[q * n + r]: order statistic r of problem q as a value
template <class T>
__global__ void sel_values_k(const SelProb* __restrict__ st, int nprob, T* __restrict__ out) {
  const int q = blockIdx.x * (64 / MAXR) + threadIdx.x / MAXR, r = threadIdx.x % MAXR;
  if (q < nprob && r < st[q].n) out[(size_t)q * st[q].n + r] = KeyOf<T>::inv((typename KeyOf<T>::K)st[q].prefix[r]);
}

// out[q]: np.median of problem q from its ranks middle_ranks<T>(count), the mean of two made in A; NaN where a value is one
template <class T, class A, class O>
__global__ void sel_median_k(const SelProb* __restrict__ st, int S, int nprob, bool seg_odd, bool uni_odd, O* __restrict__ out) {
  typedef typename KeyOf<T>::K K;
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nprob) return;
  const A lo = (A)KeyOf<T>::inv((K)st[q].prefix[0]), hi = (A)KeyOf<T>::inv((K)st[q].prefix[1]);
  const bool nan = st[q].n > 2 && (K)st[q].prefix[2] == (K)~(K)0;
  out[q] = nan ? (O)NAN : (O)median_of<A>(lo, hi, q < S ? seg_odd : uni_odd);
}

// The device-resident state of one select and the launches that advance and read it, all queued on the library stream.
template <bool UNION>
struct Select {
  int S, nprob;
  Scratch st;
  explicit Select(int S) : S(S), nprob(S + (UNION ? 1 : 0)), st((size_t)nprob * sizeof(SelProb)) {}
  bool ok() const { return st.p != nullptr; }
  unsigned blocks(int per) const { return (unsigned)((nprob + per - 1) / per); }

  // every pass over S segments of seglen values of dev; `uni`: the ranks of the union
  template <class T>
  int run(const T* dev, size_t seglen, const SelRanks& seg, const SelRanks& uni = SelRanks{}) {
    if (seg.n < 1 || seg.n > MAXR || uni.n < (UNION ? 1 : 0) || uni.n > MAXU)
      return set_error(IA3_EINVAL, "a select takes 1 to %d ranks per segment and up to %d of the union", MAXR, MAXU);
    constexpr int passes = KeyOf<T>::BITS / 8;
    const size_t pass_bins = (size_t)nprob * MAXR * NB;   // every pass has its histograms: one memset for all
    Scratch hist(passes * pass_bins * sizeof(unsigned));
    if (!hist.p) return set_error(IA3_ENOMEM, "histograms of the order statistics");
    hipStream_t s = stream();
    IA3_HIP(hipMemsetAsync(hist.p, 0, passes * pass_bins * sizeof(unsigned), s));
    hipLaunchKernelGGL(sel_init_k, dim3(blocks(64)), dim3(64), 0, s, st.as<SelProb>(), S, nprob, seg, uni);
    const size_t per_block = 256 * 64;   // values a block counts before it adds its histograms to the global ones
    size_t gx = (seglen + per_block - 1) / per_block, gmax = (size_t)num_cus() * 8 / (size_t)S;
    if (gx > gmax) gx = gmax;
    if (gx < 1) gx = 1;
    const dim3 grid((unsigned)gx, (unsigned)S);
    for (int pass = 0; pass < passes; ++pass) {
      unsigned* h = hist.as<unsigned>() + pass * pass_bins;
      hipLaunchKernelGGL((sel_hist_k<T, UNION>), grid, dim3(256), 0, s, dev, seglen, S, pass, st.as<SelProb>(), h);
      hipLaunchKernelGGL(sel_pick_k, dim3(blocks(64 / MAXR)), dim3(64), 0, s, st.as<SelProb>(), (const unsigned*)h, nprob,
                         KeyOf<T>::BITS - 8 * (pass + 1));
    }
    IA3_KCHECK();
    return IA3_OK;
  }
  // dev_out[q * n + r]: the order statistics as values
  template <class T>
  int values(T* dev_out) {
    hipLaunchKernelGGL((sel_values_k<T>), dim3(blocks(64 / MAXR)), dim3(64), 0, stream(), (const SelProb*)st.p, nprob, dev_out);
    IA3_KCHECK();
    return IA3_OK;
  }
  // dev_out[q]: the medians after run(middle_ranks<T>(seglen), middle_ranks<T>(S * seglen))
  template <class T, class A, class O>
  int medians(size_t seglen, O* dev_out) {
    hipLaunchKernelGGL((sel_median_k<T, A, O>), dim3(blocks(64)), dim3(64), 0, stream(), (const SelProb*)st.p, S, nprob,
                       seglen % 2 == 1, ((size_t)S * seglen) % 2 == 1, dev_out);
    IA3_KCHECK();
    return IA3_OK;
  }
};

// for callers that want what a select left on the device on the host: waits for the stream
template <class O>
int fetch(const O* dev, size_t n, O* host) {
  IA3_HIP(hipMemcpyAsync(host, dev, n * sizeof(O), hipMemcpyDeviceToHost, stream()));
  IA3_HIP(hipStreamSynchronize(stream()));
  return IA3_OK;
}

// np.median of each of S equally long segments, widened to float64, on the host.  kind: IA3_U16 (float64 mean of the two
// middle values for an even count), IA3_F32 (the two added and halved in float32) or IA3_SEL_F64 (in float64).  NaN for a
// segment that holds one.
inline int host_medians(const char* scope, const void* d, int kind, int S, size_t seglen, std::vector<double>& med64) {
  Select<false> sel(S);
  Scratch dmed((size_t)S * sizeof(double));
  if (!sel.ok() || !dmed.p) return set_error(IA3_ENOMEM, "scratch of the order statistics");
  double* out = dmed.as<double>();
  int rc;
  {
    ProfScope ps(scope);
    if (kind == IA3_F32) { rc = sel.run((const float*)d, seglen, middle_ranks<float>(seglen)); if (!rc) rc = sel.medians<float, float>(seglen, out); }
    else if (kind == IA3_SEL_F64) { rc = sel.run((const double*)d, seglen, middle_ranks<double>(seglen)); if (!rc) rc = sel.medians<double, double>(seglen, out); }
    else { rc = sel.run((const uint16_t*)d, seglen, middle_ranks<uint16_t>(seglen)); if (!rc) rc = sel.medians<uint16_t, double>(seglen, out); }
  }
  if (rc) return rc;
  med64.resize((size_t)S);
  return fetch(out, (size_t)S, med64.data());
}

}  // namespace
