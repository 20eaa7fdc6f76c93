// Domain distances of traced chromosomes on the device: domain_tools/distance.py of the reference.
// A population is uploaded once (ia3_domain_create): the (N, R, 3) coordinates of N chromosome copies, or one R x R distance
// map (N = 1), and optionally one R x R normalisation map.  The kernels read distances through a source, a template
// parameter: CoordSrc recomputes sqrt((dz*dz + dx*dx) + dy*dy) from the coordinates (scipy's pdist / cdist arithmetic),
// MatSrc reads entry [r, c]; both divide by norm[r, c] when the call asks for it.  No R x R map per copy exists anywhere.
//   window_k    _sliding_window_dist (:19-67): one wavefront per (copy, window size, locus).  The two sets (at most 240 and
//               256 values) are gathered into LDS in the reference's order by ballot compaction; medians by exact ranking
//               (a lane ranks its values against all of the set, read as LDS broadcasts), means and variances by NumPy's
//               pairwise order on one lane per set, the KS statistic from `<=` counts of every value in both sets.
//   dists_k     domain_distance (:69-158) for a list of (copy, s1, e1, s2, e2): one workgroup per entry runs the medians of
//               both sets side by side as radix selects by recomputation (8 digits of 8 key bits, ending once both ranks
//               are alone in their bins, then one pass that reads the value off and finds the upper middle one), then the
//               medians of (d - m)**2 the same way.
//   contacts_k  _domain_contact_freq (:465-490): one workgroup per entry counts the contacts of a block.
// LDS: window_k 4.1 KiB, dists_k 2.2 KiB per workgroup.  Integer atomics only, each value they make is a count, a maximum or
// a minimum of keys: the same bits on every run, and for every set of other entries in the call.
#include "ia3_rt.h"
#include "ia3_distsum.h"
#include "ia3_domain.h"
#include <math.h>
#include <string.h>
#include <vector>

using namespace ia3rt;
using namespace ia3dm;

namespace {

constexpr int DM_WAVE = 64;

struct DmArgs {
  const double* data;    // (N, R, 3) or (R, R)
  const double* norm;    // (R, R) or null: no division
  int N, R;
  // windows
  int W, metric;
  int wd[DM_MAX_W];
  // entries
  const int* quads;      // (Q, 5): copy, s1, e1, s2, e2
  int allow_minus;
  double th, qstar;
  double* out;
  int* flag;
};

__device__ inline double norm_of(const DmArgs& A, double v, int r, int c) {
  return A.norm ? v / A.norm[(size_t)r * A.R + c] : v;
}

struct CoordSrc {
  const double* p;
  const DmArgs& A;
  __device__ CoordSrc(const DmArgs& a, int copy) : p(a.data + (size_t)copy * a.R * 3), A(a) {}
  __device__ inline double q(int r, int c) const {
    const double dz = p[3 * r] - p[3 * c], dx = p[3 * r + 1] - p[3 * c + 1], dy = p[3 * r + 2] - p[3 * c + 2];
    return __dadd_rn(__dadd_rn(__dmul_rn(dz, dz), __dmul_rn(dx, dx)), __dmul_rn(dy, dy));
  }
  __device__ inline double at(int r, int c) const { return norm_of(A, sqrt(q(r, c)), r, c); }
  // squareform(pdist(.)) <= th: the diagonal is the literal 0, elsewhere sqrt(q) <= th is q <= q* (ia3_dist_qstar)
  __device__ inline bool contact(int r, int c) const { return r == c ? 0.0 <= A.th : q(r, c) <= A.qstar; }
};

struct MatSrc {
  const DmArgs& A;
  __device__ MatSrc(const DmArgs& a, int) : A(a) {}
  __device__ inline double at(int r, int c) const { return norm_of(A, A.data[(size_t)r * A.R + c], r, c); }
  __device__ inline bool contact(int r, int c) const { return A.data[(size_t)r * A.R + c] <= A.th; }
};

// ---- windows ----------------------------------------------------------------------------------------------------------

// np.median of v[0 .. n) by the whole wavefront (the workgroup is one); slot: two doubles of LDS
__device__ inline double wave_median(const double* v, int n, double* slot) {
  const int lo = dm_mid_lo(n), hi = dm_mid_hi(n);
  int nan = 0;
  for (int k = threadIdx.x; k < n; k += DM_WAVE) {
    const double vk = v[k];
    nan |= vk != vk ? 1 : 0;
    int r = 0;
    for (int j = 0; j < n; ++j) r += dm_before(v[j], j, vk, k) ? 1 : 0;
    if (r == lo) slot[0] = vk;
    if (r == hi) slot[1] = vk;
  }
  const int any_nan = __syncthreads_or(nan);
  const double m = any_nan ? dm_nan() : dm_median2(slot[0], slot[1], n);
  __syncthreads();
  return m;
}

template <class Src>
__global__ __launch_bounds__(DM_WAVE) void window_k(DmArgs A) {
  __shared__ double s_intra[DM_MAX_INTRA], s_inter[DM_MAX_INTER];
  __shared__ double s_slot[4];
  const int lane = threadIdx.x, R = A.R;
  const long long pb = blockIdx.x;
  const int i = (int)(pb % R), w = (int)((pb / R) % A.W), copy = (int)(pb / ((long long)R * A.W));
  const int wd = A.wd[w], metric = A.metric;
  double* out = A.out + pb;
  if (dm_edge(i, wd, R)) {
    if (lane == 0) *out = 0.0;
    return;
  }
  int l0, r1;
  dm_slices(i, wd, R, &l0, &r1);
  const Src src(A, copy);
  const unsigned long long below = (1ull << lane) - 1ull;
  int ni = 0, nj = 0;
  // rows x cols entries from (r0, c0) in row-major order, the kept ones appended to dst in that order
  auto gather = [&](int r0, int c0, int rows, int cols, bool upper, double* dst, int& cnt) {
    for (int t0 = 0; t0 < rows * cols; t0 += DM_WAVE) {
      const int t = t0 + lane;
      bool keep = false;
      double v = 0.0;
      if (t < rows * cols) {
        const int r = t / cols, c = t % cols;
        if (!upper || r < c) {
          v = src.at(r0 + r, c0 + c);
          keep = upper ? dm_keep_intra(v) : dm_keep_inter(v);
        }
      }
      const unsigned long long mask = __ballot(keep);
      if (keep) dst[cnt + __popcll(mask & below)] = v;
      cnt += __popcll(mask);
    }
  };
  gather(l0, l0, i - l0, i - l0, true, s_intra, ni);
  gather(i, i, r1 - i, r1 - i, true, s_intra, ni);
  gather(l0, i, i - l0, r1 - i, false, s_inter, nj);
  __syncthreads();
  if (ni == 0 || nj == 0) {
    if (lane == 0) *out = 0.0;
    return;
  }
  if (metric == DM_W_MEDIAN || metric == DM_W_KS) {
    const double m_inter = wave_median(s_inter, nj, s_slot), m_intra = wave_median(s_intra, ni, s_slot);
    double v_inter = 0.0, v_intra = 0.0;
    if (metric == DM_W_KS) {
      double mn = INFINITY, mx = -INFINITY;
      for (int k = lane; k < ni + nj; k += DM_WAVE) {
        const double x = k < ni ? s_intra[k] : s_inter[k - ni];
        int ca = 0, cb = 0;
        for (int j = 0; j < ni; ++j) ca += s_intra[j] <= x ? 1 : 0;
        for (int j = 0; j < nj; ++j) cb += s_inter[j] <= x ? 1 : 0;
        const double d = dm_ks_diff(ca, ni, cb, nj);
        mn = d < mn ? d : mn;
        mx = d > mx ? d : mx;
      }
      for (int o = DM_WAVE / 2; o > 0; o >>= 1) {
        const double a = __shfl_xor(mn, o), b = __shfl_xor(mx, o);
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
      }
      v_inter = dm_ks_stat(mn, mx, ni, nj);
    } else {
      for (int k = lane; k < nj; k += DM_WAVE) s_inter[k] = dm_dev2(s_inter[k], m_inter);
      for (int k = lane; k < ni; k += DM_WAVE) s_intra[k] = dm_dev2(s_intra[k], m_intra);
      __syncthreads();
      v_inter = wave_median(s_inter, nj, s_slot);
      v_intra = wave_median(s_intra, ni, s_slot);
    }
    if (lane == 0) *out = dm_window_final(metric, m_inter, m_intra, v_inter, v_intra);
    return;
  }
  // the means: lane 0 takes the inter set, lane 1 the intra set
  if (lane < 2) {
    const double* a = lane ? s_intra : s_inter;
    const int n = lane ? ni : nj;
    const double mean = dm_mean([a](int k) { return a[k]; }, n);
    s_slot[2 * lane] = mean;
    s_slot[2 * lane + 1] = metric == DM_W_MEAN ? dm_var([a](int k) { return a[k]; }, n, mean) : 0.0;
  }
  __syncthreads();
  if (lane == 0) *out = dm_window_final(metric, s_slot[0], s_slot[2], s_slot[1], s_slot[3]);
}

// ---- domain distances and contacts ------------------------------------------------------------------------------------

struct Quad {
  int copy, s1, n1, s2, n2;
  unsigned a, b, total;   // entries of the first square, of both squares, of all three blocks
  __device__ explicit Quad(const int* q) : copy(q[0]), s1(q[1]), n1(q[2] - q[1]), s2(q[3]), n2(q[4] - q[3]) {
    a = (unsigned)n1 * n1;
    b = a + (unsigned)n2 * n2;
    total = b + (unsigned)n1 * n2;
  }
};

// f(set, d) for every distance of the entry, set 0: inter (the block [s1:e1, s2:e2]), set 1: intra (the entries above the
// diagonal of the two squares); the order is that of the threads, the medians do not depend on it
template <int T, class Src, class F>
__device__ inline void visit(const Quad& Q, const Src& src, F f) {
  for (unsigned t = threadIdx.x; t < Q.total; t += T) {
    if (t < Q.a) {
      const int r = t / Q.n1, c = t % Q.n1;
      if (r < c) f(1, src.at(Q.s1 + r, Q.s1 + c));
    } else if (t < Q.b) {
      const int r = (t - Q.a) / Q.n2, c = (t - Q.a) % Q.n2;
      if (r < c) f(1, src.at(Q.s2 + r, Q.s2 + c));
    } else {
      const int r = (t - Q.b) / Q.n2, c = (t - Q.b) % Q.n2;
      f(0, src.at(Q.s1 + r, Q.s2 + c));
    }
  }
}

struct SelectLds {
  unsigned hist[2][DM_BINS];
  u64 prefix[2], lo[2], mn[2];
  unsigned k[2], c[2], le[2];
};

// np.nanmedian of val(set, d) over both sets at once: count[s] values are not NaN, med[s] is their median
template <int T, class Src, class V>
__device__ inline void select2(const Quad& Q, const Src& src, SelectLds& S, V val, unsigned count[2], double med[2]) {
  if (threadIdx.x < 2) { S.prefix[threadIdx.x] = 0; S.k[threadIdx.x] = 0; S.c[threadIdx.x] = 0; }
  int last = DM_PASSES - 1;
  for (int pass = 0; pass < DM_PASSES; ++pass) {
    for (int i = threadIdx.x; i < 2 * DM_BINS; i += T) (&S.hist[0][0])[i] = 0;
    __syncthreads();
    const u64 prefix[2] = {S.prefix[0], S.prefix[1]};
    // a thread adds a run of equal digits at once: the leading digits of distances are nearly all the same
    int cur[2] = {-1, -1};
    unsigned run[2] = {0, 0};
    visit<T>(Q, src, [&](int s, double d) {
      const double v = val(s, d);
      if (v != v) return;
      const u64 key = dm_key(v);
      if (!dm_matches(key, prefix[s], pass)) return;
      const int g = dm_digit(key, pass);
      if (g == cur[s]) { ++run[s]; return; }
      if (run[s]) atomicAdd(&S.hist[s][cur[s]], run[s]);
      cur[s] = g;
      run[s] = 1;
    });
    for (int s = 0; s < 2; ++s)
      if (run[s]) atomicAdd(&S.hist[s][cur[s]], run[s]);
    __syncthreads();
    // the bin of the rank, by the first wavefront: a half of it per set, a lane sums DM_BINS / 32 bins, a prefix sum over the
    // half names the lane whose bins hold the rank, and that lane walks them
    int more = 0;
    if (threadIdx.x < DM_WAVE) {
      constexpr int PER = DM_BINS / 32;
      const int s = threadIdx.x >> 5, l = threadIdx.x & 31;
      unsigned part = 0;
      for (int b = 0; b < PER; ++b) part += S.hist[s][l * PER + b];
      unsigned incl = part;
      for (int o = 1; o < 32; o <<= 1) {
        const unsigned t = __shfl_up(incl, o, 32);
        if (l >= o) incl += t;
      }
      unsigned k = S.k[s];
      if (pass == 0) {   // the values that are not NaN, and the lower middle rank among them
        const unsigned c = __shfl(incl, 31, 32);
        if (l == 0) S.c[s] = c;
        k = c ? (c - 1) / 2 : 0;
      }
      if (incl - part <= k && k < incl) {   // one lane, or none where the set has no value
        k -= incl - part;
        const int b = ia3ds::ds_pick_bin(S.hist[s], l * PER, PER, k);
        S.prefix[s] |= (u64)b << dm_shift(pass);
        S.k[s] = k;
        more = S.hist[s][b] > 1 ? 1 : 0;
      }
    }
    if (!__syncthreads_or(more)) { last = pass; break; }
  }
  // the lower middle value in full, the number of values <= it and the smallest value above it
  if (threadIdx.x < 2) { S.lo[threadIdx.x] = 0; S.mn[threadIdx.x] = ~0ull; S.le[threadIdx.x] = 0; }
  __syncthreads();
  const int low = dm_shift(last);
  const u64 lo_top[2] = {S.prefix[0] >> low, S.prefix[1] >> low};
  unsigned le[2] = {0, 0};
  u64 mn[2] = {~0ull, ~0ull}, lo[2] = {0, 0};
  visit<T>(Q, src, [&](int s, double d) {
    const double v = val(s, d);
    if (v != v) return;
    const u64 key = dm_key(v), top = key >> low;
    if (top <= lo_top[s]) {
      ++le[s];
      if (top == lo_top[s]) lo[s] = key;
    } else if (key < mn[s]) mn[s] = key;
  });
  for (int s = 0; s < 2; ++s) {
    if (le[s]) atomicAdd(&S.le[s], le[s]);
    if (lo[s]) atomicMax(&S.lo[s], lo[s]);
    if (mn[s] != ~0ull) atomicMin(&S.mn[s], mn[s]);
  }
  __syncthreads();
  for (int s = 0; s < 2; ++s) {
    count[s] = S.c[s];
    med[s] = dm_nanmedian(S.c[s], S.lo[s], S.le[s], S.mn[s]);
  }
  __syncthreads();
}

template <class Src, int T>
__global__ __launch_bounds__(T) void dists_k(DmArgs A) {
  __shared__ SelectLds S;
  const Quad Q(A.quads + 5 * (size_t)blockIdx.x);
  const Src src(A, Q.copy);
  unsigned n[2], n2[2];
  double m[2], v[2] = {0.0, 0.0};
  select2<T>(Q, src, S, [](int, double d) { return d; }, n, m);
  if (A.metric == DM_D_MEDIAN && n[0] && n[1])   // the same for every thread
    select2<T>(Q, src, S, [&](int s, double d) { return dm_dev2(d, m[s]); }, n2, v);
  if (threadIdx.x == 0) {
    int zero;
    A.out[blockIdx.x] = dm_dist_final(A.metric, n[0], n[1], m[0], m[1], v[0], v[1], A.allow_minus, &zero);
    A.flag[blockIdx.x] = zero;
  }
}

template <class Src, int T>
__global__ __launch_bounds__(T) void contacts_k(DmArgs A) {
  __shared__ unsigned s_count;
  const Quad Q(A.quads + 5 * (size_t)blockIdx.x);
  const Src src(A, Q.copy);
  if (threadIdx.x == 0) s_count = 0;
  __syncthreads();
  const unsigned cells = (unsigned)Q.n1 * Q.n2;
  unsigned mine = 0;
  for (unsigned t = threadIdx.x; t < cells; t += T) mine += src.contact(Q.s1 + t / Q.n2, Q.s2 + t % Q.n2) ? 1u : 0u;
  if (mine) atomicAdd(&s_count, mine);
  __syncthreads();
  if (threadIdx.x == 0) {
    A.flag[blockIdx.x] = (int)s_count;
    A.out[blockIdx.x] = (double)s_count / (double)cells;   // np.mean of no entry: 0 / 0
  }
}

constexpr unsigned DM_SMALL = 2048;   // entries of the largest quadruple up to which a workgroup is one wavefront

}  // namespace

struct ia3_domain_population {
  int N = 0, R = 0, is_matrix = 0;
  double* d = nullptr;      // one allocation: the data, then the normalisation map
  double* norm = nullptr;
};

namespace {

int check_quads(const char* who, const ia3_domain_population* h, const int* quads, int Q, unsigned* largest) {
  *largest = 0;
  for (int q = 0; q < Q; ++q) {
    const int* e = quads + 5 * (size_t)q;
    if (e[0] < 0 || e[0] >= h->N) return set_error(IA3_EINVAL, "%s: entry %d names copy %d of %d", who, q, e[0], h->N);
    if (e[1] < 0 || e[2] < e[1] || e[2] > h->R || e[3] < 0 || e[4] < e[3] || e[4] > h->R)
      return set_error(IA3_EINVAL, "%s: entry %d has bounds [%d, %d) and [%d, %d) of %d loci", who, q, e[1], e[2], e[3], e[4], h->R);
    const long long n1 = e[2] - e[1], n2 = e[4] - e[3], total = n1 * n1 + n2 * n2 + n1 * n2;   // R <= 16384: below 2^30
    if ((unsigned)total > *largest) *largest = (unsigned)total;
  }
  return IA3_OK;
}

template <class Src>
void launch_entries(bool contacts, bool small, int Q, hipStream_t st, const DmArgs& A) {
  if (contacts) {
    if (small) hipLaunchKernelGGL((contacts_k<Src, 64>), dim3((unsigned)Q), dim3(64), 0, st, A);
    else hipLaunchKernelGGL((contacts_k<Src, 256>), dim3((unsigned)Q), dim3(256), 0, st, A);
  } else {
    if (small) hipLaunchKernelGGL((dists_k<Src, 64>), dim3((unsigned)Q), dim3(64), 0, st, A);
    else hipLaunchKernelGGL((dists_k<Src, 256>), dim3((unsigned)Q), dim3(256), 0, st, A);
  }
}

int run_entries(ia3_domain_population* h, bool contacts, const int* quads, int Q, DmArgs& A, double* out, int* flag) {
  const char* who = contacts ? "domain_contacts" : "domain_dists";
  unsigned largest = 0;
  int rc = check_quads(who, h, quads, Q, &largest); if (rc) return rc;
  hipStream_t st = stream();
  Scratch d_quads((size_t)Q * 5 * sizeof(int)), d_out((size_t)Q * sizeof(double)), d_flag((size_t)Q * sizeof(int));
  if (!d_quads.p || !d_out.p || !d_flag.p) return set_error(IA3_ENOMEM, "%s: scratch for %d entries", who, Q);
  IA3_HIP(hipMemcpyAsync(d_quads.p, quads, (size_t)Q * 5 * sizeof(int), hipMemcpyHostToDevice, st));
  A.data = h->d; A.N = h->N; A.R = h->R;
  A.quads = d_quads.as<int>(); A.out = d_out.as<double>(); A.flag = d_flag.as<int>();
  {
    ProfScope ps(contacts ? "domain_contacts" : "domain_dists");
    if (h->is_matrix) launch_entries<MatSrc>(contacts, largest <= DM_SMALL, Q, st, A);
    else launch_entries<CoordSrc>(contacts, largest <= DM_SMALL, Q, st, A);
    IA3_KCHECK();
  }
  IA3_HIP(hipMemcpyAsync(out, d_out.p, (size_t)Q * sizeof(double), hipMemcpyDeviceToHost, st));
  if (flag) IA3_HIP(hipMemcpyAsync(flag, d_flag.p, (size_t)Q * sizeof(int), hipMemcpyDeviceToHost, st));
  IA3_HIP(hipStreamSynchronize(st));
  return IA3_OK;
}

}  // namespace

extern "C" {

int ia3_domain_create(const double* data, int N, int R, int is_matrix, const double* norm, void** out) {
  int rc = ensure_init(); if (rc) return rc;
  if (!out) return set_error(IA3_EINVAL, "domain_create: null handle");
  *out = nullptr;
  if (!data || N < 1 || R < 1 || (is_matrix && N != 1))
    return set_error(IA3_EINVAL, "domain_create: null data, or %d copies of %d loci%s", N, R, is_matrix ? " as a distance map (one is required)" : "");
  if (R > IA3_DOMAIN_MAX_R) return set_error(IA3_EUNSUPPORTED, "domain_create: %d loci (at most %d are built)", R, IA3_DOMAIN_MAX_R);
  const size_t n_data = is_matrix ? (size_t)R * R : (size_t)N * R * 3, n_norm = norm ? (size_t)R * R : 0;
  ia3_domain_population* h = new ia3_domain_population();
  h->N = N; h->R = R; h->is_matrix = is_matrix ? 1 : 0;
  hipError_t e = hipMalloc((void**)&h->d, (n_data + n_norm) * sizeof(double));
  if (e != hipSuccess) { delete h; return set_error(IA3_ENOMEM, "domain_create: hipMalloc of %zu bytes: %s", (n_data + n_norm) * sizeof(double), hipGetErrorString(e)); }
  hipStream_t st = stream();
  e = hipMemcpyAsync(h->d, data, n_data * sizeof(double), hipMemcpyHostToDevice, st);
  if (e == hipSuccess && norm) {
    h->norm = h->d + n_data;
    e = hipMemcpyAsync(h->norm, norm, n_norm * sizeof(double), hipMemcpyHostToDevice, st);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) { (void)hipFree(h->d); delete h; return set_error(IA3_EHIP, "domain_create: upload failed: %s", hipGetErrorString(e)); }
  *out = h;
  return IA3_OK;
}

void ia3_domain_free(void* handle) {
  ia3_domain_population* h = (ia3_domain_population*)handle;
  if (!h) return;
  (void)hipStreamSynchronize(stream());
  if (h->d) (void)hipFree(h->d);
  delete h;
}

int ia3_domain_slide_dev(void* handle, const int* window_sizes, int W, int metric, int use_norm, double* out) {
  ia3_domain_population* h = (ia3_domain_population*)handle;
  if (!h || !window_sizes || !out) return set_error(IA3_EINVAL, "domain_slide: null population, window sizes or output");
  if (W < 1 || W > IA3_DOMAIN_MAX_WINDOWS) return set_error(IA3_EINVAL, "domain_slide: %d window sizes (1 to %d)", W, IA3_DOMAIN_MAX_WINDOWS);
  if (metric < IA3_DOMAIN_WINDOW_MEDIAN || metric > IA3_DOMAIN_WINDOW_INSULATION) return set_error(IA3_EINVAL, "domain_slide: metric %d", metric);
  if (use_norm && !h->norm) return set_error(IA3_EINVAL, "domain_slide: the population holds no normalisation map");
  DmArgs A;
  memset(&A, 0, sizeof(A));
  for (int w = 0; w < W; ++w) {
    if (window_sizes[w] < 1) return set_error(IA3_EINVAL, "domain_slide: window size %d", window_sizes[w]);
    if (window_sizes[w] > IA3_DOMAIN_MAX_WINDOW)
      return set_error(IA3_EUNSUPPORTED, "domain_slide: window size %d (at most %d is built)", window_sizes[w], IA3_DOMAIN_MAX_WINDOW);
    A.wd[w] = window_sizes[w];
  }
  const long long problems = (long long)h->N * W * h->R;
  if (problems > 0x7fffffffLL) return set_error(IA3_EUNSUPPORTED, "domain_slide: %lld windows in one call", problems);
  hipStream_t st = stream();
  Scratch d_out((size_t)problems * sizeof(double));
  if (!d_out.p) return set_error(IA3_ENOMEM, "domain_slide: scratch for %lld windows", problems);
  A.data = h->d; A.norm = use_norm ? h->norm : nullptr; A.N = h->N; A.R = h->R; A.W = W; A.metric = metric;
  A.out = d_out.as<double>();
  {
    ProfScope ps("domain_slide");
    if (h->is_matrix) hipLaunchKernelGGL(window_k<MatSrc>, dim3((unsigned)problems), dim3(DM_WAVE), 0, st, A);
    else hipLaunchKernelGGL(window_k<CoordSrc>, dim3((unsigned)problems), dim3(DM_WAVE), 0, st, A);
    IA3_KCHECK();
  }
  IA3_HIP(hipMemcpyAsync(out, d_out.p, (size_t)problems * sizeof(double), hipMemcpyDeviceToHost, st));
  IA3_HIP(hipStreamSynchronize(st));
  return IA3_OK;
}

int ia3_domain_dists_dev(void* handle, const int* quads, int Q, int metric, int allow_minus, int use_norm, double* out,
                         int* int_zero) {
  ia3_domain_population* h = (ia3_domain_population*)handle;
  if (!h || !quads || !out || !int_zero) return set_error(IA3_EINVAL, "domain_dists: null population, entries or outputs");
  if (Q < 1) return set_error(IA3_EINVAL, "domain_dists: %d entries (at least one is required)", Q);
  if (metric < IA3_DOMAIN_DIST_MEDIAN || metric > IA3_DOMAIN_DIST_INSULATION) return set_error(IA3_EINVAL, "domain_dists: metric %d", metric);
  if (use_norm && !h->norm) return set_error(IA3_EINVAL, "domain_dists: the population holds no normalisation map");
  DmArgs A;
  memset(&A, 0, sizeof(A));
  A.norm = use_norm ? h->norm : nullptr;
  A.metric = metric; A.allow_minus = allow_minus ? 1 : 0;
  return run_entries(h, false, quads, Q, A, out, int_zero);
}

int ia3_domain_contacts_dev(void* handle, const int* quads, int Q, double contact_th, double* freq, int* n_contact) {
  ia3_domain_population* h = (ia3_domain_population*)handle;
  if (!h || !quads || !freq) return set_error(IA3_EINVAL, "domain_contacts: null population, entries or output");
  if (Q < 1) return set_error(IA3_EINVAL, "domain_contacts: %d entries (at least one is required)", Q);
  DmArgs A;
  memset(&A, 0, sizeof(A));
  A.th = contact_th;
  A.qstar = ia3_dist_qstar(contact_th);
  return run_entries(h, true, quads, Q, A, freq, n_contact);
}

}  // extern "C"
