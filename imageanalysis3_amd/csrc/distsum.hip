// Summaries of population distance maps on the device: structure_tools/distance.py:12-67, the stack of
// squareform(pdist(zxys)) / cdist(zxys1, zxys2) matrices of one chromosome pair reduced along the stack by np.nanmedian,
// np.nanmean or contact_prob, without the stack.  The coordinate tables of all chromosome copies are uploaded once
// (ia3_dist_create) and a summary call names N pairs of copies.
//   median_k   a workgroup owns a tile of output entries for the whole select and recomputes the tile's
//              q = (dz*dz + dx*dx) + dy*dy from coordinates staged in LDS in every pass: up to nine digit passes of 7 key
//              bits (the sign is known) with one LDS histogram per entry narrow the lower middle value down, ending as
//              soon as it is alone in its bin for every entry of the tile; one more pass reads that value off in full and
//              finds the upper one (ia3_distsum.h); lanes run over entries first, then over n.  Tiles of 2 x 2, 4 x 4 and
//              8 x 8 entries (64, 16 and 4 lanes per entry) are built
//   count_k    one lane per entry: q <= q* and finite q counted, the contact probability
//   mean_k     one lane per entry adds the roots in the order of n (np.nanmean of an (N, Ra, Rb) stack); mean1_k: the
//              pairwise order NumPy takes for Ra * Rb == 1
//   stack_contact_k   contact_prob of a stack that the caller holds
// Device memory of a summary call beyond the resident tables: 2 N ints (the pairs' places) and Ra * Rb * 16 bytes of
// outputs.  Nothing of size N * Ra * Rb exists anywhere: the per-entry state of the select (one prefix, one rank, 128
// counters) lives in LDS, 34 KiB per workgroup at the 8 x 8 tile, 8 KiB at 4 x 4.
// Integer atomics only, and every value they make is a count, so every run gives the same bits.
#include "ia3_rt.h"
#include "ia3_distsum.h"
#include <math.h>
#include <string.h>
#include <map>
#include <vector>

using namespace ia3rt;
using namespace ia3ds;

namespace {

constexpr int DS_THREADS = 256;
constexpr int DS_HSTRIDE = DS_BINS + 1;      // histogram of entry e at e * 129: lanes of a wave start on different banks

int g_tile = 0;                              // IA3_TUNE_DIST_TILE

struct DArgs {
  const double* A; const double* B;          // (place, region, column) of a group at base[(region * 3 + column) * stride + place]
  long long strideA, strideB;
  const int* placeA; const int* placeB;      // N each
  int N, Ra, Rb, same;
  double qstar;
  int want_prob;
  double* out; int* n_finite; int* n_contact;
};

__device__ inline double qnan() { return __longlong_as_double(0x7ff8000000000000LL); }

// The coordinates of a TA x TB tile for CH stack entries at a time: s[n * ROWP + column * TA + ia] of the rows,
// s[n * ROWP + 3 * TA + column * TB + ib] of the columns.  ROWP is odd: consecutive n start two banks apart.
template <int TA, int TB, int CH>
struct Tile {
  static constexpr int DS_CHUNK = CH;
  static constexpr int TE = TA * TB, NS = DS_THREADS / TE, ROW = 3 * (TA + TB), ROWP = ROW + 1;

  // a thread stages one stack entry n of the chunk (CH divides the workgroup): its two places are read once
  __device__ static inline void load(const DArgs& A, int a0, int b0, int n0, double* s) {
    static_assert(DS_THREADS % CH == 0, "a thread keeps its n over the rows of the staging loop");
    const int n = threadIdx.x % CH;
    const bool in = n0 + n < A.N;
    const long long pa = in ? A.placeA[n0 + n] : 0, pb = in ? A.placeB[n0 + n] : 0;
    for (int j = threadIdx.x / CH; j < ROW; j += DS_THREADS / CH) {
      double v = qnan();
      if (in) {
        if (j < 3 * TA) {
          const int c = j / TA, r = a0 + j % TA;
          if (r < A.Ra) v = A.A[((long long)r * 3 + c) * A.strideA + pa];
        } else {
          const int c = (j - 3 * TA) / TB, r = b0 + (j - 3 * TA) % TB;
          if (r < A.Rb) v = A.B[((long long)r * 3 + c) * A.strideB + pb];
        }
      }
      s[n * ROWP + j] = v;
    }
  }
  // scipy's pdist / cdist: every operation rounded on its own
  __device__ static inline double q(const double* s, int n, int ia, int ib) {
    const double* p = s + n * ROWP;
    const double dz = p[ia] - p[3 * TA + ib];
    const double dx = p[TA + ia] - p[3 * TA + TB + ib];
    const double dy = p[2 * TA + ia] - p[3 * TA + 2 * TB + ib];
    return __dadd_rn(__dadd_rn(__dmul_rn(dz, dz), __dmul_rn(dx, dx)), __dmul_rn(dy, dy));
  }
  // f(q) for the thread's entry and every n of its share, in the order of n; every thread of the workgroup calls this
  template <class F>
  __device__ static inline void stream(const DArgs& A, int a0, int b0, double* s, F f) {
    const int e = threadIdx.x % TE, sub = threadIdx.x / TE, ia = e / TB, ib = e % TB;
    const bool live = a0 + ia < A.Ra && b0 + ib < A.Rb;
    const bool diag = A.same && a0 + ia == b0 + ib;   // squareform's diagonal: the literal 0, NaN rows too
    for (int n0 = 0; n0 < A.N; n0 += DS_CHUNK) {
      load(A, a0, b0, n0, s);
      __syncthreads();
      const int cnt = min(DS_CHUNK, A.N - n0);
      if (live)
        for (int n = sub; n < cnt; n += NS) f(diag ? 0.0 : q(s, n, ia, ib));
      __syncthreads();
    }
  }
};

template <int TA, int TB, int CH>
__global__ __launch_bounds__(DS_THREADS) void median_k(DArgs A) {
  typedef Tile<TA, TB, CH> T;
  constexpr int DS_CHUNK = CH;
  constexpr int TE = T::TE, NS = T::NS, PER = DS_BINS / NS;   // NS threads share an entry: each scans PER bins
  __shared__ double s_xyz[DS_CHUNK * T::ROWP];
  __shared__ unsigned s_hist[TE * DS_HSTRIDE];
  __shared__ unsigned s_part[DS_THREADS];
  __shared__ u64 s_min[DS_THREADS], s_lo[DS_THREADS];
  __shared__ u64 s_prefix[TE];
  __shared__ unsigned s_k[TE], s_c[TE];
  const int a0 = blockIdx.y * TA, b0 = blockIdx.x * TB;
  const int e = threadIdx.x % TE, sub = threadIdx.x / TE;
  if (threadIdx.x < TE) { s_prefix[threadIdx.x] = DS_TOP; s_k[threadIdx.x] = 0; s_c[threadIdx.x] = 0; }
  int last = DS_PASSES - 1;   // the last digit pass that ran
  for (int pass = 0; pass < DS_PASSES; ++pass) {
    for (int i = threadIdx.x; i < TE * DS_HSTRIDE; i += DS_THREADS) s_hist[i] = 0;
    __syncthreads();
    const u64 prefix = s_prefix[e];
    unsigned* hist = s_hist + e * DS_HSTRIDE;
    T::stream(A, a0, b0, s_xyz, [&](double q) {
      if (q != q) return;
      const u64 key = ds_key(q);
      if (ds_matches(key, prefix, pass)) atomicAdd(&hist[ds_digit(key, pass)], 1u);
    });
    unsigned part = 0;
    for (int b = sub * PER; b < (sub + 1) * PER; ++b) part += hist[b];
    s_part[e * NS + sub] = part;
    __syncthreads();
    int more = 0;   // the rank's bin still holds several values
    if (sub == 0) {
      unsigned k = s_k[e];
      if (pass == 0) {   // the values that are not NaN, and the lower middle rank among them
        unsigned c = 0;
        for (int i = 0; i < NS; ++i) c += s_part[e * NS + i];
        s_c[e] = c;
        k = c ? (c - 1) / 2 : 0;
      }
      if (s_c[e]) {
        const int p = ds_pick_bin(s_part + e * NS, 0, NS, k);
        const int b = ds_pick_bin(hist, p * PER, PER, k);
        s_prefix[e] = prefix | ((u64)b << ds_shift(pass));
        s_k[e] = k;
        more = hist[b] > 1 ? 1 : 0;
      }
    }
    // once every rank of the tile is alone in its bin the decided bits name its value: the remaining digits are read off
    // that value in the last pass instead of being selected
    if (!__syncthreads_or(more)) { last = pass; break; }
  }
  // the lower middle value in full (the values that agree with it on the decided bits: one value, or equal ones) and the
  // upper middle value; below the decided bits nothing lies between the rank's value and its neighbours
  const int low = ds_shift(last);
  const u64 lo_top = s_prefix[e] >> low;
  unsigned le = 0;
  u64 mn = ~0ull, lo = 0;
  T::stream(A, a0, b0, s_xyz, [&](double q) {
    if (q != q) return;
    const u64 key = ds_key(q), top = key >> low;
    if (top <= lo_top) {
      ++le;
      if (top == lo_top) lo = key;
    } else if (key < mn) mn = key;
  });
  s_part[e * NS + sub] = le;
  s_min[e * NS + sub] = mn;
  s_lo[e * NS + sub] = lo;
  __syncthreads();
  const int ra = a0 + e / TB, rb = b0 + e % TB;
  if (sub == 0 && ra < A.Ra && rb < A.Rb) {
    for (int i = 1; i < NS; ++i) {
      le += s_part[e * NS + i];
      const u64 m = s_min[e * NS + i], l = s_lo[e * NS + i];
      mn = m < mn ? m : mn;
      lo = l > lo ? l : lo;
    }
    const unsigned c = s_c[e];
    A.out[(long long)ra * A.Rb + rb] = ds_median(c, lo, ds_upper_key(lo, c, le, mn));
  }
}

constexpr int DS_FLAT = 16;   // tile edge of the kernels with one lane per entry

__global__ __launch_bounds__(DS_THREADS) void count_k(DArgs A) {
  typedef Tile<DS_FLAT, DS_FLAT, 32> T;
  __shared__ double s_xyz[32 * T::ROWP];
  const int a0 = blockIdx.y * DS_FLAT, b0 = blockIdx.x * DS_FLAT;
  int nf = 0, nc = 0;
  const double qstar = A.qstar;
  T::stream(A, a0, b0, s_xyz, [&](double q) {
    nf += q < INFINITY ? 1 : 0;   // a finite root: q is neither NaN nor inf
    nc += q <= qstar ? 1 : 0;
  });
  const int ra = a0 + threadIdx.x / DS_FLAT, rb = b0 + threadIdx.x % DS_FLAT;
  if (ra >= A.Ra || rb >= A.Rb) return;
  const long long o = (long long)ra * A.Rb + rb;
  if (A.n_finite) A.n_finite[o] = nf;
  if (A.n_contact) A.n_contact[o] = nc;
  if (A.want_prob) A.out[o] = (double)nc / (double)nf;   // 0 / 0: NaN, n / 0: inf, as NumPy's true division
}

__global__ __launch_bounds__(DS_THREADS) void mean_k(DArgs A) {
  typedef Tile<DS_FLAT, DS_FLAT, 32> T;
  __shared__ double s_xyz[32 * T::ROWP];
  const int a0 = blockIdx.y * DS_FLAT, b0 = blockIdx.x * DS_FLAT;
  double s = 0.0;
  int cnt = 0;
  T::stream(A, a0, b0, s_xyz, [&](double q) {
    const bool nan = q != q;
    s = __dadd_rn(s, nan ? 0.0 : sqrt(q));
    cnt += nan ? 0 : 1;
  });
  const int ra = a0 + threadIdx.x / DS_FLAT, rb = b0 + threadIdx.x % DS_FLAT;
  if (ra >= A.Ra || rb >= A.Rb) return;
  A.out[(long long)ra * A.Rb + rb] = s / (double)cnt;
}

// Ra == Rb == 1: the stack axis is contiguous and NumPy adds it pairwise
__global__ void mean1_k(DArgs A) {
  if (blockIdx.x || threadIdx.x) return;
  auto q_of = [&](long long n) {
    if (A.same) return 0.0;
    const int pa = A.placeA[n], pb = A.placeB[n];
    const double dz = A.A[pa] - A.B[pb];
    const double dx = A.A[A.strideA + pa] - A.B[A.strideB + pb];
    const double dy = A.A[2 * A.strideA + pa] - A.B[2 * A.strideB + pb];
    return __dadd_rn(__dadd_rn(__dmul_rn(dz, dz), __dmul_rn(dx, dx)), __dmul_rn(dy, dy));
  };
  int cnt = 0;
  for (int n = 0; n < A.N; ++n) {
    const double q = q_of(n);
    cnt += q == q ? 1 : 0;
  }
  auto at = [&](long long n) {
    const double q = q_of(n);
    return q != q ? 0.0 : sqrt(q);
  };
  A.out[0] = ds_pairwise(at, (long long)A.N) / (double)cnt;
}

// contact_prob of an (N, K) stack the caller holds: `v <= th` on the values themselves
__global__ __launch_bounds__(DS_THREADS) void stack_contact_k(const double* __restrict__ v, long long N, long long K, double th,
                                                               double* __restrict__ prob, int* __restrict__ n_finite,
                                                               int* __restrict__ n_contact) {
  const long long k = (long long)blockIdx.x * DS_THREADS + threadIdx.x;
  if (k >= K) return;
  int nf = 0, nc = 0;
  for (long long n = 0; n < N; ++n) {
    const double x = v[n * K + k];
    nf += fabs(x) < INFINITY ? 1 : 0;
    nc += x <= th ? 1 : 0;
  }
  prob[k] = (double)nc / (double)nf;
  if (n_finite) n_finite[k] = nf;
  if (n_contact) n_contact[k] = nc;
}

}  // namespace

namespace ia3k { void set_dist_tile(int v) { g_tile = v == 2 || v == 4 || v == 8 ? v : 0; } }

// copies with the same number of rows form a group: region-major, the copies of a group side by side
struct ia3_dist_population {
  int M = 0;
  double* d = nullptr;
  std::vector<int> rows, group, place;        // per copy
  std::vector<long long> base, size;          // per group: offset of its block in d (doubles), copies in it
};

extern "C" {

int ia3_dist_create(const double* zxys, const int* copy_start, int M, ia3_dist_population** out) {
  int rc = ensure_init(); if (rc) return rc;
  if (!out) return set_error(IA3_EINVAL, "dist_create: null handle");
  *out = nullptr;
  if (M < 1 || !copy_start || copy_start[0] != 0) return set_error(IA3_EINVAL, "dist_create: %d copies, or a table that does not start at 0", M);
  for (int m = 0; m < M; ++m)
    if (copy_start[m + 1] < copy_start[m]) return set_error(IA3_EINVAL, "dist_create: copy_start falls at copy %d", m);
  const long long total = copy_start[M];
  if (total > 0 && !zxys) return set_error(IA3_EINVAL, "dist_create: null coordinates");
  ia3_dist_population* h = new ia3_dist_population();
  h->M = M;
  h->rows.resize(M); h->group.resize(M); h->place.resize(M);
  std::map<int, int> group_of_rows;
  for (int m = 0; m < M; ++m) {
    const int r = copy_start[m + 1] - copy_start[m];
    auto it = group_of_rows.find(r);
    if (it == group_of_rows.end()) { it = group_of_rows.emplace(r, (int)h->size.size()).first; h->size.push_back(0); }
    h->rows[m] = r; h->group[m] = it->second; h->place[m] = (int)h->size[it->second]++;
  }
  h->base.resize(h->size.size());
  std::vector<int> rows_of_group(h->size.size());
  for (int m = 0; m < M; ++m) rows_of_group[h->group[m]] = h->rows[m];
  long long off = 0;
  for (size_t g = 0; g < h->size.size(); ++g) { h->base[g] = off; off += h->size[g] * rows_of_group[g] * 3; }
  std::vector<double> host((size_t)(off > 0 ? off : 1));
  for (int m = 0; m < M; ++m) {
    const long long b = h->base[h->group[m]], stride = h->size[h->group[m]];
    const double* src = zxys + (size_t)copy_start[m] * 3;
    for (int r = 0; r < h->rows[m]; ++r)
      for (int c = 0; c < 3; ++c) host[(size_t)(b + ((long long)r * 3 + c) * stride + h->place[m])] = src[(size_t)r * 3 + c];
  }
  hipError_t e = hipMalloc((void**)&h->d, host.size() * sizeof(double));
  if (e != hipSuccess) { delete h; return set_error(IA3_ENOMEM, "dist_create: hipMalloc of %zu bytes: %s", host.size() * sizeof(double), hipGetErrorString(e)); }
  hipStream_t st = stream();
  e = hipMemcpyAsync(h->d, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) { (void)hipFree(h->d); delete h; return set_error(IA3_EHIP, "dist_create: upload failed: %s", hipGetErrorString(e)); }
  *out = h;
  return IA3_OK;
}

void ia3_dist_free(ia3_dist_population* h) {
  if (!h) return;
  (void)hipStreamSynchronize(stream());
  if (h->d) (void)hipFree(h->d);
  delete h;
}

int ia3_dist_summary_dev(ia3_dist_population* h, const int* pair_a, const int* pair_b, int N, int Ra, int Rb, int same,
                         int function, double contact_th, double* out, int* n_finite, int* n_contact) {
  if (!h || !pair_a || !pair_b || !out) return set_error(IA3_EINVAL, "dist_summary: null population, pairs or output");
  if (N < 1) return set_error(IA3_EINVAL, "dist_summary: %d pairs (at least one is required)", N);
  if (Ra < 1 || Rb < 1 || (same && Ra != Rb)) return set_error(IA3_EINVAL, "dist_summary: a %d x %d summary%s", Ra, Rb, same ? " of a copy with itself" : "");
  if (function != IA3_DIST_NANMEDIAN && function != IA3_DIST_NANMEAN && function != IA3_DIST_CONTACT)
    return set_error(IA3_EINVAL, "dist_summary: function %d", function);
  std::vector<int> place((size_t)2 * N);
  for (int n = 0; n < N; ++n) {
    const int a = pair_a[n], b = pair_b[n];
    if (a < 0 || a >= h->M || b < 0 || b >= h->M) return set_error(IA3_EINVAL, "dist_summary: pair %d names copies %d and %d of %d", n, a, b, h->M);
    if (h->rows[a] != Ra || h->rows[b] != Rb)
      return set_error(IA3_EINVAL, "dist_summary: pair %d has %d x %d rows, the summary %d x %d", n, h->rows[a], h->rows[b], Ra, Rb);
    if (same && a != b) return set_error(IA3_EINVAL, "dist_summary: pair %d is not a copy with itself", n);
    place[n] = h->place[a];
    place[(size_t)N + n] = h->place[b];
  }
  const int ga = h->group[pair_a[0]], gb = h->group[pair_b[0]];   // equal rows: one group per side
  const size_t K = (size_t)Ra * Rb;
  const bool counts = function == IA3_DIST_CONTACT || n_finite || n_contact;
  hipStream_t st = stream();
  Scratch d_place((size_t)2 * N * sizeof(int)), d_out(K * sizeof(double)), d_cnt(2 * K * sizeof(int));
  if (!d_place.p || !d_out.p || !d_cnt.p) return set_error(IA3_ENOMEM, "dist_summary: scratch for %d pairs and %zu entries", N, K);
  IA3_HIP(hipMemcpyAsync(d_place.p, place.data(), (size_t)2 * N * sizeof(int), hipMemcpyHostToDevice, st));
  DArgs A;
  A.A = h->d + h->base[ga]; A.B = h->d + h->base[gb];
  A.strideA = h->size[ga]; A.strideB = h->size[gb];
  A.placeA = d_place.as<int>(); A.placeB = d_place.as<int>() + N;
  A.N = N; A.Ra = Ra; A.Rb = Rb; A.same = same ? 1 : 0;
  A.qstar = ia3_dist_qstar(contact_th);
  A.want_prob = function == IA3_DIST_CONTACT ? 1 : 0;
  A.out = d_out.as<double>();
  A.n_finite = d_cnt.as<int>(); A.n_contact = d_cnt.as<int>() + K;
  const dim3 flat((unsigned)((Rb + DS_FLAT - 1) / DS_FLAT), (unsigned)((Ra + DS_FLAT - 1) / DS_FLAT));
  if (flat.y > 65535u) return set_error(IA3_EUNSUPPORTED, "dist_summary: %d rows (at most %d are built)", Ra, 65535 * 2);
  if (function == IA3_DIST_NANMEDIAN) {
    ProfScope ps("dist_median");
    // the 2 x 2 tile has 64 lanes per entry: it fills the device where the 4 x 4 tiles are fewer than two per CU
    const long long tiles4 = (long long)((Ra + 3) / 4) * ((Rb + 3) / 4);
    const int tile = g_tile ? g_tile : (tiles4 < 2LL * num_cus() ? 2 : 4);
    const dim3 grid((unsigned)((Rb + tile - 1) / tile), (unsigned)((Ra + tile - 1) / tile));
    if (grid.y > 65535u) return set_error(IA3_EUNSUPPORTED, "dist_summary: %d rows (at most %d are built)", Ra, 65535 * 2);
    if (tile == 2) hipLaunchKernelGGL((median_k<2, 2, 256>), grid, dim3(DS_THREADS), 0, st, A);
    else if (tile == 4) hipLaunchKernelGGL((median_k<4, 4, 64>), grid, dim3(DS_THREADS), 0, st, A);
    else hipLaunchKernelGGL((median_k<8, 8, 32>), grid, dim3(DS_THREADS), 0, st, A);
    IA3_KCHECK();
  } else if (function == IA3_DIST_NANMEAN) {
    ProfScope ps("dist_mean");
    if (K == 1) hipLaunchKernelGGL(mean1_k, dim3(1), dim3(64), 0, st, A);
    else hipLaunchKernelGGL(mean_k, flat, dim3(DS_THREADS), 0, st, A);
    IA3_KCHECK();
  }
  if (counts) {
    ProfScope ps("dist_count");
    hipLaunchKernelGGL(count_k, flat, dim3(DS_THREADS), 0, st, A);
    IA3_KCHECK();
  }
  IA3_HIP(hipMemcpyAsync(out, d_out.p, K * sizeof(double), hipMemcpyDeviceToHost, st));
  if (n_finite) IA3_HIP(hipMemcpyAsync(n_finite, A.n_finite, K * sizeof(int), hipMemcpyDeviceToHost, st));
  if (n_contact) IA3_HIP(hipMemcpyAsync(n_contact, A.n_contact, K * sizeof(int), hipMemcpyDeviceToHost, st));
  IA3_HIP(hipStreamSynchronize(st));
  return IA3_OK;
}

int ia3_dist_contact_stack_dev(const double* stack, long long N, long long K, double contact_th, double* prob, int* n_finite,
                               int* n_contact) {
  int rc = ensure_init(); if (rc) return rc;
  if (!stack || !prob || N < 1 || K < 1) return set_error(IA3_EINVAL, "dist_contact_stack: a %lld x %lld stack or a null table", N, K);
  if (N > 0x7fffffffLL || K > (1LL << 31) * DS_THREADS / 2 || N > (1LL << 60) / K)
    return set_error(IA3_EUNSUPPORTED, "dist_contact_stack: a %lld x %lld stack", N, K);
  hipStream_t st = stream();
  Scratch d_v((size_t)N * K * sizeof(double)), d_p((size_t)K * sizeof(double)), d_c((size_t)2 * K * sizeof(int));
  if (!d_v.p || !d_p.p || !d_c.p) return set_error(IA3_ENOMEM, "dist_contact_stack: scratch for a %lld x %lld stack", N, K);
  IA3_HIP(hipMemcpyAsync(d_v.p, stack, (size_t)N * K * sizeof(double), hipMemcpyHostToDevice, st));
  {
    ProfScope ps("dist_stack_contact");
    hipLaunchKernelGGL(stack_contact_k, dim3((unsigned)((K + DS_THREADS - 1) / DS_THREADS)), dim3(DS_THREADS), 0, st, d_v.as<double>(), N, K,
                       contact_th, d_p.as<double>(), d_c.as<int>(), d_c.as<int>() + K);
    IA3_KCHECK();
  }
  IA3_HIP(hipMemcpyAsync(prob, d_p.p, (size_t)K * sizeof(double), hipMemcpyDeviceToHost, st));
  if (n_finite) IA3_HIP(hipMemcpyAsync(n_finite, d_c.as<int>(), (size_t)K * sizeof(int), hipMemcpyDeviceToHost, st));
  if (n_contact) IA3_HIP(hipMemcpyAsync(n_contact, d_c.as<int>() + K, (size_t)K * sizeof(int), hipMemcpyDeviceToHost, st));
  IA3_HIP(hipStreamSynchronize(st));
  return IA3_OK;
}

}  // extern "C"
