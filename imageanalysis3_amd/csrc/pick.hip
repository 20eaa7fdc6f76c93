// Population spot picking on the device: spot_tools/picking.py:1567-2342, the path of
// pick_spots_by_intensities, generate_reference_from_population (E-step), pick_spots_by_scores (M-step) and
// evaluate_differences, on a population that is uploaded once and stays resident over the EM iterations.
//   intensity_k   one lane per (chromosome, region): the first row of maximal h (np.argmax: the first NaN wins)
//   center_k      one lane per (chromosome, key, column): np.nanmean of the picked rows / of all candidate rows, added in
//                 row order (no tree, no prefix sums); the candidates' centres are made once and kept in the handle
//   estep_k       one lane per (chromosome, region): centre distance, local-centre distance and intensity of the picked row,
//                 and the non-NaN values appended to the reference arrays (per channel and 'all'): places by wavefront
//                 ballot and an LDS count, one global atomic per workgroup and array
//   (rocPRIM radix sort of every reference array; sorted float64 values do not depend on the sort that made them)
//   mstep_k       one lane per (chromosome, region): the lane walks its candidates, so the first maximum needs no cross-lane
//                 step; three cum_val searches per candidate whose first 8 levels read pivots staged in LDS
//   difference_k  the two counts of evaluate_differences
// Arithmetic (all of it is the contract): a 2-D candidate table takes sqrt((dz*dz + dx*dx) + dy*dy), a 1-D row (every
// picked row, and a region given as one 1-D row) takes BLAS ddot's sqrt(fma(dy, dy, fma(dx, dx, dz*dz))); both are written
// with explicit roundings.  np.log is not evaluated here: a search carries the heap number of the node it ends on and the
// host supplies the log of that node's mid (ia3.h).
#include "ia3_rt.h"
#include "ia3_wave.h"
#include <math.h>
#include <string.h>
#include <rocprim/rocprim.hpp>
#include <vector>

using namespace ia3rt;

namespace {

constexpr int PK_THREADS = 256;
constexpr int PK_KEYS = IA3_PICK_MAX_CHANNELS + 1;   // channels and 'all' (the key after the last channel)
constexpr int PK_PIV = 256;                          // heap numbers 1..255: the first 8 levels of a search
constexpr int PK_LDS_LEVELS = 8;

struct Table { double* d; int n; int cap; bool owned; };   // one sorted reference array

__device__ inline double qnan() { return __longlong_as_double(0x7ff8000000000000LL); }

// np.linalg.norm(a, axis=1) over three columns
__device__ inline double norm_plain(double dz, double dx, double dy) {
  return sqrt(__dadd_rn(__dadd_rn(__dmul_rn(dz, dz), __dmul_rn(dx, dx)), __dmul_rn(dy, dy)));
}
// np.linalg.norm of a 1-D 3-vector: sqrt(ddot(a, a))
__device__ inline double norm_ddot(double dz, double dx, double dy) {
  return sqrt(__fma_rn(dy, dy, __fma_rn(dx, dx, __dmul_rn(dz, dz))));
}

// np.nanmean of rows added one after the other: the first row starts the sum, a NaN counts as 0
struct NanMean {
  double s = 0;
  int cnt = 0;
  bool first = true;
  __device__ inline void add(double v) {
    const bool nan = v != v;
    const double x = nan ? 0.0 : v;
    s = first ? x : __dadd_rn(s, x);
    first = false;
    cnt += nan ? 0 : 1;
  }
  __device__ inline double mean() const { return s / (double)cnt; }   // 0 / 0: NaN, as nanmean of no value
};

// pivot of heap node idx (1..255) of the search in tab[0..n): NaN when the search cannot reach that node
__device__ inline double pivot_of(const double* __restrict__ tab, int n, int idx) {
  if (n < 1) return qnan();
  int m = 0, M = n - 1;
  const int depth = 31 - __clz(idx);
  for (int b = depth - 1; b >= 0; --b) {
    const int mid = (m + M) >> 1;
    if ((idx >> b) & 1) m = mid; else M = mid;
    if (M - m < 2) return qnan();
  }
  return tab[(m + M) >> 1];
}

struct Found { int mid, node; };
// picking.py:1879-1899 cum_val, literally: the mid of the last iteration and the heap number of that iteration's node
// (root 1, a true compare goes to 2 * node + 1).  n >= 1.  piv: the pivots of nodes 1..255 in LDS.
__device__ inline Found cum_search(const double* __restrict__ tab, int n, const double* piv, double t) {
  int m = 0, M = n - 1, node = 1, it = 0;
  Found f;
  for (;;) {
    f.mid = (m + M) >> 1;
    f.node = node;
    const double v = it < PK_LDS_LEVELS ? piv[node] : tab[f.mid];
    const bool lt = v < t;
    if (lt) m = f.mid; else M = f.mid;
    node = 2 * node + (lt ? 1 : 0);
    ++it;
    if (M - m < 2 || it > 15) break;
  }
  return f;
}

__global__ __launch_bounds__(PK_THREADS) void cum_vals_k(const double* __restrict__ tab, int n, const double* __restrict__ targets,
                                                          int m, int* __restrict__ mids) {
  __shared__ double s_piv[PK_PIV];
  for (int i = threadIdx.x; i < PK_PIV; i += PK_THREADS) s_piv[i] = i ? pivot_of(tab, n, i) : 0.0;
  __syncthreads();
  for (int i = blockIdx.x * PK_THREADS + threadIdx.x; i < m; i += gridDim.x * PK_THREADS)
    mids[i] = cum_search(tab, n, s_piv, targets[i]).mid;
}

__global__ __launch_bounds__(PK_THREADS) void intensity_k(const double* __restrict__ cand, const int* __restrict__ start, int PR,
                                                           double* __restrict__ picks, int* __restrict__ pick_idx) {
  const int e = blockIdx.x * PK_THREADS + threadIdx.x;
  if (e >= PR) return;
  const int a = start[e], b = start[e + 1];
  int best = -1;
  double bh = 0;
  bool nan = false;
  for (int r = a; r < b && !nan; ++r) {
    const double h = cand[(size_t)r * 4];
    if (h != h) { best = r; nan = true; }
    else if (best < 0 || h > bh) { best = r; bh = h; }
  }
  for (int c = 0; c < 4; ++c) picks[(size_t)e * 4 + c] = best < 0 ? qnan() : cand[(size_t)best * 4 + c];
  pick_idx[e] = best < 0 ? -1 : best - a;
}

// ctr[(p * nk + k) * 3 + c]: nanmean of column 1 + c over the rows of chromosome p in the regions of key k (nk == 1: all
// regions).  start == nullptr: rows is a P*R x 4 table of picks, otherwise the candidate table with its CSR.
__global__ void center_k(const double* __restrict__ rows, const int* __restrict__ start, const int* __restrict__ chan, int P, int R,
                         int nk, double* __restrict__ ctr) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P * nk * 3) return;
  const int c = i % 3, k = (i / 3) % nk, p = i / (3 * nk);
  NanMean nm;
  for (int j = 0; j < R; ++j) {
    if (nk > 1 && chan[j] != k) continue;
    const int e = p * R + j;
    const int a = start ? start[e] : e, b = start ? start[e + 1] : e + 1;
    for (int r = a; r < b; ++r) nm.add(rows[(size_t)r * 4 + 1 + c]);
  }
  ctr[i] = nm.mean();
}

// centres given by the caller: one z, x, y per chromosome for every key
__global__ void center_given_k(const double* __restrict__ given, int P, int nk, double* __restrict__ ctr) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P * nk * 3) return;
  ctr[i] = given[(i / (3 * nk)) * 3 + i % 3];
}

// np.nanmean of the window's reference rows (picking.py:1689-1704), columns z, x, y
__device__ inline void local_center(const double* __restrict__ ref, int p, int R, const int* __restrict__ win_idx, int w0, int w1,
                                    double out[3]) {
  NanMean nm[3];
  for (int w = w0; w < w1; ++w) {
    const double* q = ref + ((size_t)p * R + win_idx[w]) * 4;
    for (int c = 0; c < 3; ++c) nm[c].add(q[1 + c]);
  }
  for (int c = 0; c < 3; ++c) out[c] = nm[c].mean();
}

struct EArgs {
  const double* picks; const double* ref; const double* ctr;
  const int* chan; const int* win_start; const int* win_idx;
  int P, R, nch, split;
  double* out[3];            // ct, lc, int per (chromosome, region)
  double* seg[3];            // channel segments of the three reference arrays
  double* all[3];
  long long seg_off[PK_KEYS];
  int* cnt;                  // [3][PK_KEYS]
};

// Appending to the reference arrays, one global atomic per workgroup and array: every wavefront reserves its share of
// the workgroup's count in LDS (ia3::wave_append), the workgroup's total takes a place in the array with one atomic, and
// the lanes store behind it.  Every lane of the workgroup must take every step.
__global__ __launch_bounds__(PK_THREADS) void estep_k(EArgs A) {
  __shared__ int s_count[3 * PK_KEYS], s_base[3 * PK_KEYS];
  const int PR = A.P * A.R;
  const int span = (PR + PK_THREADS - 1) / PK_THREADS * PK_THREADS;   // whole workgroups: every lane reaches every barrier
  for (int e = blockIdx.x * PK_THREADS + threadIdx.x; e < span; e += gridDim.x * PK_THREADS) {
    const bool live = e < PR;
    double v[3] = {0, 0, 0};
    int ch = -1;
    if (threadIdx.x < 3 * PK_KEYS) s_count[threadIdx.x] = 0;
    if (live) {
      const int p = e / A.R, j = e % A.R;
      ch = A.chan[j];
      const double* row = A.picks + (size_t)e * 4;
      const double* c = A.ctr + ((size_t)p * (A.split ? A.nch : 1) + (A.split ? ch : 0)) * 3;
      v[0] = norm_ddot(row[1] - c[0], row[2] - c[1], row[3] - c[2]);
      double lc[3];
      local_center(A.ref, p, A.R, A.win_idx, A.win_start[j], A.win_start[j + 1], lc);
      v[1] = norm_ddot(row[1] - lc[0], row[2] - lc[1], row[3] - lc[2]);
      v[2] = row[0];
      for (int k = 0; k < 3; ++k) A.out[k][e] = v[k];
    }
    __syncthreads();
    int own[3], all[3];   // the lane's places in its channel's array and in 'all', per kind
    for (int k = 0; k < 3; ++k) {
      const bool ok = live && v[k] == v[k];
      own[k] = 0;
      if (A.split)
        for (int c = 0; c < A.nch; ++c) {
          const int sl = ia3::wave_append(s_count + k * PK_KEYS + c, ok && ch == c);
          if (ch == c) own[k] = sl;
        }
      all[k] = ia3::wave_append(s_count + k * PK_KEYS + A.nch, ok);
    }
    __syncthreads();
    if (threadIdx.x < 3 * PK_KEYS && s_count[threadIdx.x] > 0)
      s_base[threadIdx.x] = atomicAdd(A.cnt + threadIdx.x, s_count[threadIdx.x]);
    __syncthreads();
    for (int k = 0; k < 3; ++k) {
      if (!(live && v[k] == v[k])) continue;
      if (A.split) A.seg[k][A.seg_off[ch] + s_base[k * PK_KEYS + ch] + own[k]] = v[k];
      A.all[k][s_base[k * PK_KEYS + A.nch] + all[k]] = v[k];
    }
    __syncthreads();   // s_count and s_base are reused by the next pass
  }
}

struct MArgs {
  const double* cand; const int* start; const unsigned char* flag;
  const double* ref; const double* ctr;
  const int* chan; const int* win_start; const int* win_idx;
  int P, R, nch, split_int, split_dist, dist_only;
  double cw, lw;
  const double* tab[3][PK_KEYS]; int tn[3][PK_KEYS];       // sorted reference arrays: kind 0 centre, 1 local, 2 intensity
  const double* logtab[3][PK_KEYS]; int logn[3][PK_KEYS];  // log of the node's mid per heap number
  double* newpicks; double* sel_score; int* pick_idx;
  double* score; int* mids; double* cdist;                 // per candidate: score, 3 mids (ct, lc, int), 2 distances
};

__global__ __launch_bounds__(PK_THREADS) void mstep_k(MArgs A) {
  extern __shared__ __attribute__((aligned(16))) double s_piv[];   // [slot][PK_PIV]
  const int nki = A.split_int ? A.nch : 1, nkd = A.split_dist ? A.nch : 1;
  if (!A.dist_only) {
    // slots: intensity keys, then centre keys, then local keys
    const int slots = nki + 2 * nkd;
    for (int i = threadIdx.x; i < slots * PK_PIV; i += PK_THREADS) {
      const int s = i / PK_PIV, idx = i % PK_PIV;
      int kind, key;
      if (s < nki) { kind = 2; key = A.split_int ? s : A.nch; }
      else if (s < nki + nkd) { kind = 0; key = A.split_dist ? s - nki : A.nch; }
      else { kind = 1; key = A.split_dist ? s - nki - nkd : A.nch; }
      const bool used = kind == 2 || (kind == 0 ? A.cw != 0 : A.lw != 0);
      s_piv[i] = idx && used ? pivot_of(A.tab[kind][key], A.tn[kind][key], idx) : 0.0;
    }
    __syncthreads();
  }
  const int PR = A.P * A.R;
  for (int e = blockIdx.x * PK_THREADS + threadIdx.x; e < PR; e += gridDim.x * PK_THREADS) {
    const int p = e / A.R, j = e % A.R;
    const int a = A.start[e], b = A.start[e + 1];
    const int ch = A.chan[j];
    const int ki = A.split_int ? ch : A.nch, kd = A.split_dist ? ch : A.nch;
    const int si = A.split_int ? ch : 0, sd = A.split_dist ? ch : 0;
    double lc[3] = {0, 0, 0};
    const double* c = A.ctr + ((size_t)p * nkd + sd) * 3;
    const double cz = c[0], cx = c[1], cy = c[2];
    if (b > a) local_center(A.ref, p, A.R, A.win_idx, A.win_start[j], A.win_start[j + 1], lc);
    const bool one_d = A.flag[e] != 0;
    int best = -1;
    bool best_nan = false;
    double best_sc = 0, mx = qnan();
    for (int r = a; r < b; ++r) {
      const double* q = A.cand + (size_t)r * 4;
      const double h = q[0], z = q[1], x = q[2], y = q[3];
      const double dct = one_d ? norm_ddot(z - cz, x - cx, y - cy) : norm_plain(z - cz, x - cx, y - cy);
      const double dlc = one_d ? norm_ddot(z - lc[0], x - lc[1], y - lc[2]) : norm_plain(z - lc[0], x - lc[1], y - lc[2]);
      A.cdist[(size_t)r * 2] = dct;
      A.cdist[(size_t)r * 2 + 1] = dlc;
      if (A.dist_only) continue;
      int m3[3] = {-1, -1, -1};
      Found f = cum_search(A.tab[2][ki], A.tn[2][ki], s_piv + si * PK_PIV, h);
      m3[2] = f.mid;
      double sc = f.node < A.logn[2][ki] ? A.logtab[2][ki][f.node] : qnan();
      if (A.cw != 0) {
        f = cum_search(A.tab[0][kd], A.tn[0][kd], s_piv + (nki + sd) * PK_PIV, dct);
        m3[0] = f.mid;
        sc = __dadd_rn(sc, __dmul_rn(A.cw, f.node < A.logn[0][kd] ? A.logtab[0][kd][f.node] : qnan()));
      }
      if (A.lw != 0) {
        f = cum_search(A.tab[1][kd], A.tn[1][kd], s_piv + (nki + nkd + sd) * PK_PIV, dlc);
        m3[1] = f.mid;
        sc = __dadd_rn(sc, __dmul_rn(A.lw, f.node < A.logn[1][kd] ? A.logtab[1][kd][f.node] : qnan()));
      }
      A.score[r] = sc;
      for (int k = 0; k < 3; ++k) A.mids[(size_t)r * 3 + k] = m3[k];
      // np.argmax: the first NaN, otherwise the first maximum; np.nanmax: the maximum of what is not NaN
      if (sc != sc) {
        if (!best_nan) { best = r; best_nan = true; }
      } else {
        if (!best_nan && (best < 0 || sc > best_sc)) { best = r; best_sc = sc; }
        if (mx != mx || sc > mx) mx = sc;
      }
    }
    if (A.dist_only) continue;
    for (int k = 0; k < 4; ++k) A.newpicks[(size_t)e * 4 + k] = best < 0 ? qnan() : A.cand[(size_t)best * 4 + k];
    A.sel_score[e] = mx;
    A.pick_idx[e] = best < 0 ? -1 : best - a;
  }
}

__global__ __launch_bounds__(PK_THREADS) void difference_k(const double* __restrict__ a, const double* __restrict__ b, int PR,
                                                            int* __restrict__ out) {
  __shared__ int s_count[2];
  if (threadIdx.x < 2) s_count[threadIdx.x] = 0;
  __syncthreads();
  int near = 0, num = 0;
  for (int e = blockIdx.x * PK_THREADS + threadIdx.x; e < PR; e += gridDim.x * PK_THREADS) {
    const double* p = a + (size_t)e * 4;
    const double* q = b + (size_t)e * 4;
    const double d = norm_plain(p[1] - q[1], p[2] - q[2], p[3] - q[3]);
    near += d < 0.01 ? 1 : 0;
    num += d == d ? 1 : 0;
  }
  if (near) atomicAdd(&s_count[0], near);
  if (num) atomicAdd(&s_count[1], num);
  __syncthreads();
  if (threadIdx.x < 2 && s_count[threadIdx.x]) atomicAdd(out + threadIdx.x, s_count[threadIdx.x]);
}

inline unsigned blocks_for(long long n) {
  long long b = (n + PK_THREADS - 1) / PK_THREADS;
  const long long cap = (long long)num_cus() * 8;
  if (cap >= 1 && b > cap) b = cap;
  return (unsigned)(b < 1 ? 1 : b);
}

int dev_alloc(void** p, size_t bytes) {
  *p = nullptr;
  hipError_t e = hipMalloc(p, bytes ? bytes : 8);
  if (e != hipSuccess) { *p = nullptr; return set_error(IA3_ENOMEM, "hipMalloc of %zu bytes: %s", bytes, hipGetErrorString(e)); }
  return IA3_OK;
}

}  // namespace

struct ia3_pick_population {
  int P = 0, R = 0, n = 0, nch = 0;
  long long PR = 0;
  std::vector<void*> blocks;   // everything below that this handle owns
  double* cand = nullptr; int* start = nullptr; unsigned char* flag = nullptr; int* chan = nullptr;
  double* rows[3] = {nullptr, nullptr, nullptr};   // picks, previous picks, the M-step's output (rotated)
  double* ref = nullptr;                           // uploaded reference rows
  double* ctr = nullptr;                           // P x keys x 3
  double* cand_ctr = nullptr;                      // the same of all candidates (they never change): made once per layout
  int cand_ctr_keys = 0;                           // keys per chromosome that cand_ctr holds (0: not made)
  double* given = nullptr;                         // P x 3
  int* win_start = nullptr; int* win_idx = nullptr; size_t win_cap = 0;
  double* eout[3] = {nullptr, nullptr, nullptr};
  double* seg[3] = {nullptr, nullptr, nullptr};
  double* all[3] = {nullptr, nullptr, nullptr};
  double* sorttmp = nullptr;
  void* sort_scratch = nullptr; size_t sort_scratch_bytes = 0;
  int* cnt = nullptr;                              // [3][PK_KEYS] and two counts of the difference
  long long seg_off[PK_KEYS] = {0};
  int seg_cap[PK_KEYS] = {0};
  Table tab[3][PK_KEYS] = {};
  double* logtab[3][PK_KEYS] = {}; int logcap[3][PK_KEYS] = {};
  int log_for_n[3][PK_KEYS] = {}; int log_size[3][PK_KEYS] = {};   // length of the array the resident log table was made for
  double* sel_score = nullptr; int* pick_idx = nullptr;
  double* score = nullptr; int* mids = nullptr; double* cdist = nullptr;

  int take(void** p, size_t bytes) {
    int rc = dev_alloc(p, bytes);
    if (rc == IA3_OK) blocks.push_back(*p);
    return rc;
  }
};

namespace {

int upload_window(ia3_pick_population* h, const int* win_start, const int* win_idx, hipStream_t st) {
  if (!win_start || win_start[0] != 0) return set_error(IA3_EINVAL, "pick: the window table should start at 0");
  const int R = h->R;
  for (int j = 0; j < R; ++j)
    if (win_start[j + 1] < win_start[j]) return set_error(IA3_EINVAL, "pick: the window table falls at region %d", j);
  const int nw = win_start[R];
  if (nw > 0 && !win_idx) return set_error(IA3_EINVAL, "pick: null window indices");
  for (int w = 0; w < nw; ++w)
    if (win_idx[w] < 0 || win_idx[w] >= R) return set_error(IA3_EINVAL, "pick: window index %d outside 0..%d", win_idx[w], R - 1);
  if ((size_t)nw > h->win_cap) {
    void* p;
    int rc = h->take(&p, (size_t)nw * sizeof(int)); if (rc) return rc;
    h->win_idx = (int*)p;
    h->win_cap = (size_t)nw;
  }
  IA3_HIP(hipMemcpyAsync(h->win_start, win_start, (size_t)(R + 1) * sizeof(int), hipMemcpyHostToDevice, st));
  if (nw > 0) IA3_HIP(hipMemcpyAsync(h->win_idx, win_idx, (size_t)nw * sizeof(int), hipMemcpyHostToDevice, st));
  IA3_HIP(hipStreamSynchronize(st));   // the caller's tables may go away when the step returns
  return IA3_OK;
}

// the chromosome centres of every key: given by the caller, or the nanmean of `rows` (picks: start == nullptr)
int centers(ia3_pick_population* h, const double* given, const double* rows, const int* start, int nk, hipStream_t st,
            double* ctr) {
  const int total = h->P * nk * 3;
  const unsigned blocks = (unsigned)((total + 63) / 64);
  if (given) {
    IA3_HIP(hipMemcpyAsync(h->given, given, (size_t)h->P * 3 * sizeof(double), hipMemcpyHostToDevice, st));
    IA3_HIP(hipStreamSynchronize(st));
    hipLaunchKernelGGL(center_given_k, dim3(blocks), dim3(64), 0, st, h->given, h->P, nk, ctr);
  } else {
    hipLaunchKernelGGL(center_k, dim3(blocks), dim3(64), 0, st, rows, start, h->chan, h->P, h->R, nk, ctr);
  }
  IA3_KCHECK();
  return IA3_OK;
}

// in place as far as the caller sees: sorted into sorttmp and copied back, all queued on the stream; rocPRIM's scratch is a
// block of the handle that only grows (it is used by one sort at a time, in stream order)
int sort_table(ia3_pick_population* h, double* d, int n, hipStream_t st) {
  if (n < 2) return IA3_OK;
  size_t tb = 0;
  IA3_HIP(rocprim::radix_sort_keys(nullptr, tb, d, h->sorttmp, (size_t)n, 0, 64, st));
  if (tb > h->sort_scratch_bytes) {
    void* p;
    int rc = h->take(&p, tb); if (rc) return rc;
    h->sort_scratch = p;
    h->sort_scratch_bytes = tb;
  }
  IA3_HIP(rocprim::radix_sort_keys(h->sort_scratch, tb, d, h->sorttmp, (size_t)n, 0, 64, st));
  IA3_HIP(hipMemcpyAsync(d, h->sorttmp, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st));
  return IA3_OK;
}

}  // namespace

extern "C" {

int ia3_pick_create(const double* cands, int n, const int* region_start, const unsigned char* row_1d, int P, int R,
                    const int* channel, int n_channels, ia3_pick_population** out) {
  int rc = ensure_init(); if (rc) return rc;
  if (!out) return set_error(IA3_EINVAL, "pick_create: null handle");
  *out = nullptr;
  if (P < 1 || R < 1 || n < 0 || !region_start || !row_1d || (n > 0 && !cands))
    return set_error(IA3_EINVAL, "pick_create: %d chromosomes, %d regions, %d candidates or a null table", P, R, n);
  if ((long long)P * R > (1LL << 28) || n > (1 << 29))
    return set_error(IA3_EUNSUPPORTED, "pick_create: %d x %d regions, %d candidates: at most 2^28 regions and 2^29 rows are built", P, R, n);
  if (n_channels < 0 || n_channels > IA3_PICK_MAX_CHANNELS || (n_channels > 0 && !channel))
    return set_error(IA3_EINVAL, "pick_create: %d channels (at most %d)", n_channels, IA3_PICK_MAX_CHANNELS);
  const int PR = P * R;
  if (region_start[0] != 0 || region_start[PR] != n) return set_error(IA3_EINVAL, "pick_create: region_start should run from 0 to %d", n);
  for (int e = 0; e < PR; ++e) {
    if (region_start[e + 1] < region_start[e]) return set_error(IA3_EINVAL, "pick_create: region_start falls at entry %d", e);
    if (row_1d[e] && region_start[e + 1] - region_start[e] != 1) return set_error(IA3_EINVAL, "pick_create: entry %d is flagged 1-D but has not one row", e);
  }
  std::vector<int> chan(R, 0), per(PK_KEYS, 0);
  for (int j = 0; j < R && n_channels > 0; ++j) {
    if (channel[j] < 0 || channel[j] >= n_channels) return set_error(IA3_EINVAL, "pick_create: channel %d of region %d", channel[j], j);
    chan[j] = channel[j];
    per[chan[j]] += 1;
  }
  ia3_pick_population* h = new ia3_pick_population();
  h->P = P; h->R = R; h->n = n; h->nch = n_channels; h->PR = PR;
  long long off = 0;
  for (int c = 0; c < n_channels; ++c) { h->seg_off[c] = off; h->seg_cap[c] = P * per[c]; off += (long long)P * per[c]; }
  const size_t rb = (size_t)PR * 4 * sizeof(double), vb = (size_t)PR * sizeof(double), nn = (size_t)(n > 0 ? n : 1);
  void* p = nullptr;
  rc = h->take(&p, nn * 4 * sizeof(double)); h->cand = (double*)p;
  if (!rc) { rc = h->take(&p, (size_t)(PR + 1) * sizeof(int)); h->start = (int*)p; }
  if (!rc) { rc = h->take(&p, (size_t)PR); h->flag = (unsigned char*)p; }
  if (!rc) { rc = h->take(&p, (size_t)R * sizeof(int)); h->chan = (int*)p; }
  for (int k = 0; k < 3 && !rc; ++k) { rc = h->take(&p, rb); h->rows[k] = (double*)p; }
  if (!rc) { rc = h->take(&p, rb); h->ref = (double*)p; }
  if (!rc) { rc = h->take(&p, (size_t)P * PK_KEYS * 3 * sizeof(double)); h->ctr = (double*)p; }
  if (!rc) { rc = h->take(&p, (size_t)P * PK_KEYS * 3 * sizeof(double)); h->cand_ctr = (double*)p; }
  if (!rc) { rc = h->take(&p, (size_t)P * 3 * sizeof(double)); h->given = (double*)p; }
  if (!rc) { rc = h->take(&p, (size_t)(R + 1) * sizeof(int)); h->win_start = (int*)p; }
  for (int k = 0; k < 3 && !rc; ++k) {
    rc = h->take(&p, vb); h->eout[k] = (double*)p;
    if (!rc) { rc = h->take(&p, vb); h->seg[k] = (double*)p; }
    if (!rc) { rc = h->take(&p, vb); h->all[k] = (double*)p; }
  }
  if (!rc) { rc = h->take(&p, vb); h->sorttmp = (double*)p; }
  if (!rc) { rc = h->take(&p, (size_t)(3 * PK_KEYS + 2) * sizeof(int)); h->cnt = (int*)p; }
  if (!rc) { rc = h->take(&p, vb); h->sel_score = (double*)p; }
  if (!rc) { rc = h->take(&p, (size_t)PR * sizeof(int)); h->pick_idx = (int*)p; }
  if (!rc) { rc = h->take(&p, nn * sizeof(double)); h->score = (double*)p; }
  if (!rc) { rc = h->take(&p, nn * 3 * sizeof(int)); h->mids = (int*)p; }
  if (!rc) { rc = h->take(&p, nn * 2 * sizeof(double)); h->cdist = (double*)p; }
  if (rc) { ia3_pick_free(h); return rc; }
  for (int k = 0; k < 3; ++k)
    for (int c = 0; c <= n_channels; ++c)
      h->tab[k][c] = Table{c < n_channels ? h->seg[k] + h->seg_off[c] : h->all[k], 0, c < n_channels ? h->seg_cap[c] : PR, false};
  hipStream_t st = stream();
  hipError_t e = hipSuccess;
  if (n > 0) e = hipMemcpyAsync(h->cand, cands, (size_t)n * 4 * sizeof(double), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(h->start, region_start, (size_t)(PR + 1) * sizeof(int), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(h->flag, row_1d, (size_t)PR, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(h->chan, chan.data(), (size_t)R * sizeof(int), hipMemcpyHostToDevice, st);
  for (int k = 0; k < 3 && e == hipSuccess; ++k) e = hipMemsetAsync(h->rows[k], 0xff, rb, st);   // NaN rows until something is picked
  if (e == hipSuccess) e = hipMemsetAsync(h->ref, 0xff, rb, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) {
    ia3_pick_free(h);
    return set_error(IA3_EHIP, "pick_create: upload failed: %s", hipGetErrorString(e));
  }
  *out = h;
  return IA3_OK;
}

void ia3_pick_free(ia3_pick_population* h) {
  if (!h) return;
  (void)hipStreamSynchronize(stream());
  for (void* p : h->blocks) (void)hipFree(p);
  for (int k = 0; k < 3; ++k)
    for (int c = 0; c < PK_KEYS; ++c)
      if (h->tab[k][c].owned) (void)hipFree(h->tab[k][c].d);
  delete h;
}

int ia3_pick_by_intensity_dev(ia3_pick_population* h) {
  if (!h) return set_error(IA3_EINVAL, "pick: null population");
  hipStream_t st = stream();
  ProfScope ps("pick_intensity");
  hipLaunchKernelGGL(intensity_k, dim3((unsigned)((h->PR + PK_THREADS - 1) / PK_THREADS)), dim3(PK_THREADS), 0, st, h->cand, h->start,
                     (int)h->PR, h->rows[0], h->pick_idx);
  IA3_KCHECK();
  return IA3_OK;
}

int ia3_pick_set_rows(ia3_pick_population* h, int which, const double* rows) {
  if (!h || !rows || which < 0 || which > 2) return set_error(IA3_EINVAL, "pick_set_rows: null table or table %d", which);
  double* d = which == IA3_PICK_ROWS_REF ? h->ref : h->rows[which == IA3_PICK_ROWS_PREV ? 1 : 0];
  hipStream_t st = stream();
  IA3_HIP(hipMemcpyAsync(d, rows, (size_t)h->PR * 4 * sizeof(double), hipMemcpyHostToDevice, st));
  IA3_HIP(hipStreamSynchronize(st));
  return IA3_OK;
}

int ia3_pick_reference_dev(ia3_pick_population* h, const int* win_start, const int* win_idx, int split, const double* centers_zxy,
                           int ref_is_picks, int* lengths) {
  if (!h || !lengths) return set_error(IA3_EINVAL, "pick_reference: null population or lengths");
  if (split && h->nch < 1) return set_error(IA3_EINVAL, "pick_reference: channels are split but the population has none");
  hipStream_t st = stream();
  int rc = upload_window(h, win_start, win_idx, st); if (rc) return rc;
  const int nk = split ? h->nch : 1;
  std::vector<int> cnt(3 * PK_KEYS, 0);
  {
    ProfScope ps("pick_estep");
    rc = centers(h, centers_zxy, h->rows[0], nullptr, nk, st, h->ctr); if (rc) return rc;
    IA3_HIP(hipMemsetAsync(h->cnt, 0, (size_t)3 * PK_KEYS * sizeof(int), st));
    EArgs A;
    A.picks = h->rows[0]; A.ref = ref_is_picks ? h->rows[0] : h->ref; A.ctr = h->ctr;
    A.chan = h->chan; A.win_start = h->win_start; A.win_idx = h->win_idx;
    A.P = h->P; A.R = h->R; A.nch = h->nch; A.split = split ? 1 : 0;
    for (int k = 0; k < 3; ++k) { A.out[k] = h->eout[k]; A.seg[k] = h->seg[k]; A.all[k] = h->all[k]; }
    for (int c = 0; c < PK_KEYS; ++c) A.seg_off[c] = h->seg_off[c];
    A.cnt = h->cnt;
    hipLaunchKernelGGL(estep_k, dim3(blocks_for(h->PR)), dim3(PK_THREADS), 0, st, A);
    IA3_KCHECK();
  }
  IA3_HIP(hipMemcpyAsync(cnt.data(), h->cnt, (size_t)3 * PK_KEYS * sizeof(int), hipMemcpyDeviceToHost, st));
  IA3_HIP(hipStreamSynchronize(st));
  {
    ProfScope ps("pick_sort");
    for (int k = 0; k < 3; ++k)
      for (int c = 0; c < PK_KEYS; ++c) {
        if (h->tab[k][c].owned) { (void)hipFree(h->tab[k][c].d); h->tab[k][c].owned = false; }
        const bool made = c == h->nch || (split && c < h->nch);
        const int len = made ? cnt[k * PK_KEYS + c] : 0;
        if (len > (c < h->nch ? h->seg_cap[c] : (int)h->PR)) return set_error(IA3_EHIP, "pick_reference: %d values in an array of %d", len, c < h->nch ? h->seg_cap[c] : (int)h->PR);
        h->tab[k][c] = Table{c < h->nch ? h->seg[k] + h->seg_off[c] : h->all[k], len, c < h->nch ? h->seg_cap[c] : (int)h->PR, false};
        lengths[k * PK_KEYS + c] = made ? len : -1;
        if (made) { rc = sort_table(h, h->tab[k][c].d, len, st); if (rc) return rc; }
      }
  }
  return IA3_OK;
}

int ia3_pick_set_sorted(ia3_pick_population* h, int kind, int key, const double* values, int n) {
  if (!h || kind < 0 || kind > 2 || key < 0 || key > h->nch || n < 0 || (n > 0 && !values))
    return set_error(IA3_EINVAL, "pick_set_sorted: kind %d, key %d, %d values", kind, key, n);
  Table& t = h->tab[kind][key];
  if (t.owned) { (void)hipStreamSynchronize(stream()); (void)hipFree(t.d); t = Table{nullptr, 0, 0, false}; }
  void* p;
  int rc = dev_alloc(&p, (size_t)n * sizeof(double)); if (rc) return rc;
  t = Table{(double*)p, n, n, true};
  hipStream_t st = stream();
  if (n > 0) IA3_HIP(hipMemcpyAsync(t.d, values, (size_t)n * sizeof(double), hipMemcpyHostToDevice, st));
  IA3_HIP(hipStreamSynchronize(st));
  return IA3_OK;
}

int ia3_pick_scores_dev(ia3_pick_population* h, const int* win_start, const int* win_idx, int split_int, int split_dist,
                        double center_weight, double local_weight, const double* centers_zxy, int ref_is_picks,
                        const double* const* logtabs, const int* logsizes, int dist_only) {
  if (!h) return set_error(IA3_EINVAL, "pick_scores: null population");
  if ((split_int || split_dist) && h->nch < 1) return set_error(IA3_EINVAL, "pick_scores: channels are split but the population has none");
  if (!dist_only && (!logtabs || !logsizes)) return set_error(IA3_EINVAL, "pick_scores: null log tables");
  hipStream_t st = stream();
  int rc = upload_window(h, win_start, win_idx, st); if (rc) return rc;
  const int nki = split_int ? h->nch : 1, nkd = split_dist ? h->nch : 1;
  MArgs A;
  memset(&A, 0, sizeof(A));
  bool uploaded = false;
  if (!dist_only) {
    for (int k = 0; k < 3; ++k) {
      const bool used = k == 2 || (k == 0 ? center_weight != 0 : local_weight != 0);
      const bool split = k == 2 ? split_int : split_dist;
      for (int c = 0; c <= h->nch && used; ++c) {
        if (split ? c == h->nch : c != h->nch) continue;
        const int i = k * PK_KEYS + c;
        if (h->tab[k][c].n < 1) return set_error(IA3_EINVAL, "pick_scores: reference array %d of key %d is empty", k, c);
        if (!logtabs[i] || logsizes[i] < 2) return set_error(IA3_EINVAL, "pick_scores: no log table for array %d of key %d", k, c);
        if (logsizes[i] > h->logcap[k][c]) {
          void* p;
          rc = h->take(&p, (size_t)logsizes[i] * sizeof(double)); if (rc) return rc;
          h->logtab[k][c] = (double*)p;
          h->logcap[k][c] = logsizes[i];
          h->log_for_n[k][c] = -1;
        }
        // the table is a function of the array's length alone: it goes up when that length is new
        if (h->log_for_n[k][c] != h->tab[k][c].n || h->log_size[k][c] != logsizes[i]) {
          IA3_HIP(hipMemcpyAsync(h->logtab[k][c], logtabs[i], (size_t)logsizes[i] * sizeof(double), hipMemcpyHostToDevice, st));
          h->log_for_n[k][c] = h->tab[k][c].n;
          h->log_size[k][c] = logsizes[i];
          uploaded = true;
        }
        A.tab[k][c] = h->tab[k][c].d; A.tn[k][c] = h->tab[k][c].n;
        A.logtab[k][c] = h->logtab[k][c]; A.logn[k][c] = logsizes[i];
      }
    }
  }
  if (uploaded) IA3_HIP(hipStreamSynchronize(st));   // the log tables are the caller's
  ProfScope ps(dist_only ? "pick_dists" : "pick_mstep");
  if (centers_zxy) {
    rc = centers(h, centers_zxy, nullptr, nullptr, nkd, st, h->ctr); if (rc) return rc;
  } else if (h->cand_ctr_keys != nkd) {
    rc = centers(h, nullptr, h->cand, h->start, nkd, st, h->cand_ctr); if (rc) return rc;
    h->cand_ctr_keys = nkd;
  }
  A.cand = h->cand; A.start = h->start; A.flag = h->flag;
  A.ref = ref_is_picks ? h->rows[0] : h->ref; A.ctr = centers_zxy ? h->ctr : h->cand_ctr;
  A.chan = h->chan; A.win_start = h->win_start; A.win_idx = h->win_idx;
  A.P = h->P; A.R = h->R; A.nch = h->nch; A.split_int = split_int ? 1 : 0; A.split_dist = split_dist ? 1 : 0;
  A.dist_only = dist_only ? 1 : 0;
  A.cw = center_weight; A.lw = local_weight;
  A.newpicks = h->rows[2]; A.sel_score = h->sel_score; A.pick_idx = h->pick_idx;
  A.score = h->score; A.mids = h->mids; A.cdist = h->cdist;
  const size_t lds = dist_only ? 0 : (size_t)(nki + 2 * nkd) * PK_PIV * sizeof(double);
  hipLaunchKernelGGL(mstep_k, dim3(blocks_for(h->PR)), dim3(PK_THREADS), lds, st, A);
  IA3_KCHECK();
  if (!dist_only) {   // previous <- picks <- new
    double* old = h->rows[1];
    h->rows[1] = h->rows[0]; h->rows[0] = h->rows[2]; h->rows[2] = old;
  }
  return IA3_OK;
}

int ia3_pick_difference_dev(ia3_pick_population* h, int* counts) {
  if (!h || !counts) return set_error(IA3_EINVAL, "pick_difference: null population or counts");
  hipStream_t st = stream();
  int* d = h->cnt + 3 * PK_KEYS;
  {
    ProfScope ps("pick_difference");
    IA3_HIP(hipMemsetAsync(d, 0, 2 * sizeof(int), st));
    hipLaunchKernelGGL(difference_k, dim3(blocks_for(h->PR)), dim3(PK_THREADS), 0, st, h->rows[1], h->rows[0], (int)h->PR, d);
    IA3_KCHECK();
  }
  IA3_HIP(hipMemcpyAsync(counts, d, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
  IA3_HIP(hipStreamSynchronize(st));
  return IA3_OK;
}

int ia3_pick_download(ia3_pick_population* h, int what, void* out) {
  if (!h || !out) return set_error(IA3_EINVAL, "pick_download: null population or buffer");
  const size_t PR = (size_t)h->PR, n = (size_t)h->n;
  const void* src = nullptr;
  size_t bytes = 0;
  switch (what) {
    case IA3_PICK_GET_PICKS: src = h->rows[0]; bytes = PR * 4 * sizeof(double); break;
    case IA3_PICK_GET_PREV: src = h->rows[1]; bytes = PR * 4 * sizeof(double); break;
    case IA3_PICK_GET_SEL_SCORES: src = h->sel_score; bytes = PR * sizeof(double); break;
    case IA3_PICK_GET_PICK_INDEX: src = h->pick_idx; bytes = PR * sizeof(int); break;
    case IA3_PICK_GET_SCORES: src = h->score; bytes = n * sizeof(double); break;
    case IA3_PICK_GET_MIDS: src = h->mids; bytes = n * 3 * sizeof(int); break;
    case IA3_PICK_GET_CAND_DISTS: src = h->cdist; bytes = n * 2 * sizeof(double); break;
    case IA3_PICK_GET_REF_CT: src = h->eout[0]; bytes = PR * sizeof(double); break;
    case IA3_PICK_GET_REF_LOCAL: src = h->eout[1]; bytes = PR * sizeof(double); break;
    case IA3_PICK_GET_REF_INT: src = h->eout[2]; bytes = PR * sizeof(double); break;
    default: return set_error(IA3_EINVAL, "pick_download: table %d", what);
  }
  hipStream_t st = stream();
  if (bytes) IA3_HIP(hipMemcpyAsync(out, src, bytes, hipMemcpyDeviceToHost, st));
  IA3_HIP(hipStreamSynchronize(st));
  return IA3_OK;
}

int ia3_pick_download_sorted(ia3_pick_population* h, int kind, int key, double* out) {
  if (!h || kind < 0 || kind > 2 || key < 0 || key > h->nch) return set_error(IA3_EINVAL, "pick_download_sorted: kind %d, key %d", kind, key);
  const Table& t = h->tab[kind][key];
  hipStream_t st = stream();
  if (t.n > 0) {
    if (!out) return set_error(IA3_EINVAL, "pick_download_sorted: null buffer");
    IA3_HIP(hipMemcpyAsync(out, t.d, (size_t)t.n * sizeof(double), hipMemcpyDeviceToHost, st));
  }
  IA3_HIP(hipStreamSynchronize(st));
  return IA3_OK;
}

int ia3_pick_cum_vals_dev(const double* sorted_vals, int n, const double* targets, int m, int* mids) {
  int rc = ensure_init(); if (rc) return rc;
  if (n < 1 || !sorted_vals) return set_error(IA3_EINVAL, "pick_cum_vals: %d sorted values (at least one is required)", n);
  if (m < 0 || (m > 0 && (!targets || !mids))) return set_error(IA3_EINVAL, "pick_cum_vals: %d targets or a null table", m);
  if (m == 0) return IA3_OK;
  hipStream_t st = stream();
  Scratch d_tab((size_t)n * sizeof(double)), d_t((size_t)m * sizeof(double)), d_m((size_t)m * sizeof(int));
  if (!d_tab.p || !d_t.p || !d_m.p) return set_error(IA3_ENOMEM, "pick_cum_vals: scratch for %d values and %d targets", n, m);
  IA3_HIP(hipMemcpyAsync(d_tab.p, sorted_vals, (size_t)n * sizeof(double), hipMemcpyHostToDevice, st));
  IA3_HIP(hipMemcpyAsync(d_t.p, targets, (size_t)m * sizeof(double), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(cum_vals_k, dim3(blocks_for(m)), dim3(PK_THREADS), 0, st, d_tab.as<double>(), n, d_t.as<double>(), m, d_m.as<int>());
  IA3_KCHECK();
  IA3_HIP(hipMemcpyAsync(mids, d_m.p, (size_t)m * sizeof(int), hipMemcpyDeviceToHost, st));
  IA3_HIP(hipStreamSynchronize(st));
  return IA3_OK;
}

}  // extern "C"
