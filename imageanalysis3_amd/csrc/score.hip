// Chromosomal spot scores on the device: spot_tools/scoring.py of the reference.
// A population of C traced chromosomes is uploaded once (ia3_score_create) as CSR: per chromosome its candidate rows and its
// currently selected rows, (h, z, x, y) float64 with a region id each.  Both tables get an index by region id, built on the
// device: a stable radix sort (rocPRIM) of the keys (chromosome, id) carries the row numbers along, so a chromosome's rows
// stay in its own stretch, ordered by id and, for equal ids, by row.  A region's rows are then one binary search away.
//   center_k   per chromosome np.nanmean(sel_zxys, axis=0), one accumulator per column in row order, and the centre in nm
//   geom_k     one lane per row of a table (candidates for the scores, selected rows for the references): the centre
//              distance, _local_distance against the selected rows and the forward / reverse medians of
//              neighboring_distances among the table's own rows, all by the serial text of ia3_score.h; medians by exact
//              ranking with the distances recomputed (at most 64 rows of a region: no array per lane)
//   ref_k      one wavefront per (chromosome, reference array): drops the NaNs by ballot compaction in row order, puts the
//              fallback value where nothing is left, sorts by exact ranking into a second array and reduces (nanmedian from
//              the sorted values, nanmean in NumPy's pairwise order, radius of gyration)
//   score_k    one lane per (candidate, score): upper-bound searches in the chromosome's sorted reference, the _cum_prob
//              arithmetic, and the value and class byte that the host's np.log finishes
//   lists_k    neighboring_distances(use_median=False)
// No atomics and no LDS; every value is made by one lane from the inputs alone, so a chromosome gives the same bits alone
// and inside any batch, on every run.
#include "ia3_rt.h"
#include "ia3_score.h"
#include <rocprim/rocprim.hpp>
#include <math.h>
#include <string.h>
#include <algorithm>
#include <vector>

using namespace ia3rt;
using namespace ia3sc;

namespace {

typedef unsigned long long u64;
constexpr int SC_WAVE = 64, SC_BLOCK = 256;

// one table of rows with its index
struct Table {
  const double* rows;    // (n, 4)
  const int* id;         // (n) in row order
  const int* start;      // (C + 1)
  const int* sid;        // (n) ids in index order
  const int* perm;       // (n) rows in index order
  int n;
};

struct ScArgs {
  Table tgt, sel;
  int C;
  const double* dzxy;         // 3
  const double* center_px;    // (C, 3) or null
  const int* has_center;      // (C) or null
  double* selmean;            // (C, 3) nm
  double* center;             // (C, 3) nm
  int half;
  long long step;
  double invalid, intensity_th;
  double* geom;               // (5, tgt.n): ct, lc, fwd, rev, nb
  double* inten;              // (tgt.n) filtered intensities, or null
  int n_geom;
};

__device__ inline RowIndex index_of(const Table& t, const double* dzxy, int c) {
  RowIndex r;
  r.rows = t.rows; r.sid = t.sid; r.perm = t.perm; r.dzxy = dzxy; r.lo = t.start[c]; r.hi = t.start[c + 1];
  return r;
}

__global__ __launch_bounds__(SC_BLOCK) void keys_k(const int* id, const int* start, int C, int n, u64* key, int* row) {
  const int i = blockIdx.x * SC_BLOCK + threadIdx.x;
  if (i >= n) return;
  key[i] = ((u64)(unsigned)sc_chrom_of(start, C, i) << 32) | (u64)((unsigned)id[i] ^ 0x80000000u);
  row[i] = i;
}

__global__ __launch_bounds__(SC_BLOCK) void unkey_k(const u64* key, int n, int* sid) {
  const int i = blockIdx.x * SC_BLOCK + threadIdx.x;
  if (i < n) sid[i] = (int)((unsigned)key[i] ^ 0x80000000u);
}

__global__ __launch_bounds__(SC_WAVE) void center_k(ScArgs A) {
  const int c = blockIdx.x * SC_WAVE + threadIdx.x;
  if (c >= A.C) return;
  Mean3 mean;
  for (int i = A.sel.start[c]; i < A.sel.start[c + 1]; ++i) {
    double v[3];
    sc_zxy(A.sel.rows + 4 * (size_t)i, A.dzxy, v);
    mean.add(v);
  }
  double m[3];
  mean.finish(m);
  const bool given = A.center_px && A.has_center && A.has_center[c];
  for (int k = 0; k < 3; ++k) {
    A.selmean[3 * c + k] = m[k];
    A.center[3 * c + k] = given ? A.center_px[3 * c + k] * A.dzxy[k] : m[k];
  }
}

__global__ __launch_bounds__(SC_BLOCK) void geom_k(ScArgs A) {
  const int i = blockIdx.x * SC_BLOCK + threadIdx.x;
  if (i >= A.tgt.n) return;
  const int c = sc_chrom_of(A.tgt.start, A.C, i);
  const double* row = A.tgt.rows + 4 * (size_t)i;
  double t[3];
  sc_zxy(row, A.dzxy, t);
  const long long id = A.tgt.id[i];
  const size_t n = (size_t)A.tgt.n;
  const double* ctr = A.center + 3 * c;
  A.geom[i] = sc_norm_rows(t[0] - ctr[0], t[1] - ctr[1], t[2] - ctr[2]);
  A.geom[n + i] = sc_local(t, id, A.half, A.invalid, index_of(A.sel, A.dzxy, c));
  double fwd, rev;
  sc_neighbors(t, id, A.step, A.invalid, index_of(A.tgt, A.dzxy, c), &fwd, &rev);
  A.geom[2 * n + i] = fwd;
  A.geom[3 * n + i] = rev;
  A.geom[4 * n + i] = sc_nanmean2(fwd, rev);
  if (A.inten) A.inten[i] = row[0] <= A.intensity_th ? sc_nan() : row[0];
}

struct ListArgs {
  ScArgs A;
  const int* off_fwd;
  const int* off_rev;
  double* fwd;
  double* rev;
};

__global__ __launch_bounds__(SC_BLOCK) void lists_k(ListArgs L) {
  const ScArgs& A = L.A;
  const int i = blockIdx.x * SC_BLOCK + threadIdx.x;
  if (i >= A.tgt.n) return;
  const int c = sc_chrom_of(A.tgt.start, A.C, i);
  double t[3];
  sc_zxy(A.tgt.rows + 4 * (size_t)i, A.dzxy, t);
  const long long id = A.tgt.id[i];
  const RowIndex idx = index_of(A.tgt, A.dzxy, c);
  // a value goes only where the caller's offsets leave room for it
  const int f0 = L.off_fwd[i], f1 = L.off_fwd[i + 1], r0 = L.off_rev[i], r1 = L.off_rev[i + 1];
  int b, e;
  idx.range(id + A.step, &b, &e);
  if (e <= b) {
    if (f0 < f1) L.fwd[f0] = A.invalid;
    if (r0 < r1) L.rev[r0] = A.invalid;
    return;
  }
  for (int k = b; k < e && f0 + (k - b) < f1; ++k) L.fwd[f0 + (k - b)] = sqrt(sc_q(idx, k, t));
  idx.range(id - A.step, &b, &e);
  for (int k = b; k < e && r0 + (k - b) < r1; ++k) L.rev[r0 + (k - b)] = sqrt(sc_q(idx, k, t));
}

struct RefArgs {
  int C, n_arr, stride;       // arrays of `stride` values each
  const int* start;           // (C + 1) stretches
  const double* raw;          // (n_arr, stride)
  double* comp;               // (n_arr, stride) what the reference keeps, in row order
  double* sorted;             // (n_arr, stride) the values that are not NaN, ascending
  int* counts;                // (C, n_arr) values of comp; -1: one value, the reference's fallback
  int* m;                     // (C, n_arr) values of sorted
  double* scalars;            // (C, n_arr)
  int ignore_nan, fallback, metric;
  // the radius of gyration
  const double* rows;
  const double* dzxy;
  const double* selmean;
};

__device__ inline double fallback_of(int a) { return a == 0 ? 1000.0 : (a == 3 ? 1.0 : sc_inf()); }

__global__ __launch_bounds__(SC_WAVE) void ref_k(RefArgs R) {
  const int lane = threadIdx.x, p = blockIdx.x, c = p / R.n_arr, a = p % R.n_arr;
  const int lo = R.start[c], n = R.start[c + 1] - lo;
  const size_t base = (size_t)a * R.stride + lo;
  const double* raw = R.raw + base;
  double* comp = R.comp + base;
  double* sorted = R.sorted + base;
  const unsigned long long below = (1ull << lane) - 1ull;
  int cnt = 0;
  bool fell_back = false;
  if (R.ignore_nan) {
    for (int t0 = 0; t0 < n; t0 += SC_WAVE) {
      const int t = t0 + lane;
      const double v = t < n ? raw[t] : sc_nan();
      const bool keep = v == v;
      const unsigned long long mask = __ballot(keep);
      if (keep) comp[cnt + __popcll(mask & below)] = v;
      cnt += __popcll(mask);
    }
    if (cnt == 0 && R.fallback && n > 0) {
      if (lane == 0) comp[0] = fallback_of(a);
      cnt = 1;
      fell_back = true;
    }
  } else {
    for (int t = lane; t < n; t += SC_WAVE) comp[t] = raw[t];
    cnt = n;
  }
  __syncthreads();
  int m = 0;
  for (int k0 = 0; k0 < cnt; k0 += SC_WAVE) {
    const int k = k0 + lane;
    const double vk = k < cnt ? comp[k] : sc_nan();
    const bool real = vk == vk;
    if (real) {
      int r = 0;
      for (int j = 0; j < cnt; ++j) r += ia3dm::dm_before(comp[j], j, vk, k) ? 1 : 0;
      sorted[r] = vk;
    }
    m += __popcll(__ballot(real));
  }
  __syncthreads();
  if (lane != 0) return;
  R.counts[p] = fell_back ? -1 : cnt;   // -1: the one value is the fallback
  R.m[p] = m;
  double s = sc_nan();
  if (R.metric == SC_REF_MEDIAN) s = sc_median_sorted(sorted, m);
  else if (R.metric == SC_REF_MEAN) s = sc_nanmean_1d([comp](int i) { return comp[i]; }, cnt);
  else if (R.metric == SC_REF_RG && a < 3) {
    const double* rows = R.rows + 4 * (size_t)lo;
    const double* dz = R.dzxy;
    s = sc_rg([rows, dz](int i, double* v) { sc_zxy(rows + 4 * (size_t)i, dz, v); }, n, R.selmean + 3 * c);
  }
  R.scalars[p] = s;
}

struct ScoreArgs {
  int C, N, S;                 // chromosomes, values per score, stride of the sorted arrays
  const int* tgt_start;        // (C + 1) or null: one chromosome
  const int* ref_start;        // (C + 1)
  const double* x[4];          // (N) each
  int n_scores, kind[4];
  double w[4], lo[4], hi[4];
  const double* scalars;       // (C, n_scores)
  const double* sorted;        // (n_scores, S)
  const int* m;                // (C, n_scores)
  int x_stride;                // elements between consecutive values of x (4 for the intensity column of a row table)
  double* val;                 // (n_scores, N)
  unsigned char* cls;
};

__global__ __launch_bounds__(SC_BLOCK) void score_k(ScoreArgs A) {
  const long long g = (long long)blockIdx.x * SC_BLOCK + threadIdx.x;
  if (g >= (long long)A.N * A.n_scores) return;
  const int a = (int)(g / A.N), i = (int)(g % A.N);
  const int c = A.tgt_start ? sc_chrom_of(A.tgt_start, A.C, i) : 0;
  const double x = A.x[a][(size_t)i * (a == 3 ? A.x_stride : 1)];
  const int p = c * A.n_scores + a;
  int cls;
  const double v = sc_score(A.kind[a], x, A.scalars[p], A.sorted + (size_t)a * A.S + A.ref_start[c], A.m[p], A.w[a], A.lo[a], A.hi[a], &cls);
  A.val[g] = v;
  A.cls[g] = (unsigned char)cls;
}

template <class T>
int dev_alloc(T** p, size_t n, const char* who) {
  *p = nullptr;
  hipError_t e = hipMalloc((void**)p, (n ? n : 1) * sizeof(T));
  if (e != hipSuccess) { *p = nullptr; return set_error(IA3_ENOMEM, "%s: hipMalloc of %zu bytes: %s", who, n * sizeof(T), hipGetErrorString(e)); }
  return IA3_OK;
}

struct DevTable {
  double* rows = nullptr;
  int *id = nullptr, *start = nullptr, *sid = nullptr, *perm = nullptr;
  int n = 0;
  std::vector<int> h_start;
  void release() {
    for (void* p : {(void*)rows, (void*)id, (void*)start, (void*)sid, (void*)perm}) if (p) (void)hipFree(p);
    rows = nullptr; id = start = sid = perm = nullptr; n = 0;
  }
  Table view() const { Table t; t.rows = rows; t.id = id; t.start = start; t.sid = sid; t.perm = perm; t.n = n; return t; }
};

inline unsigned blocks(long long n, int per) { return (unsigned)((n + per - 1) / per); }

// the offsets ascend from 0, every chromosome has a row, every id lies in int32 and no region id of a chromosome has more
// than IA3_SCORE_MAX_PER_REGION rows; ids32: the ids as int32
int check_table(const char* who, const char* what, const long long* id, const int* start, int C, std::vector<int>& ids32) {
  if (start[0] != 0) return set_error(IA3_EINVAL, "%s: the %s offsets start at %d", who, what, start[0]);
  for (int c = 0; c < C; ++c)
    if (start[c + 1] <= start[c]) return set_error(IA3_EINVAL, "%s: chromosome %d has no %s row", who, c, what);
  const int n = start[C];
  ids32.resize((size_t)n);
  for (int i = 0; i < n; ++i) {
    if (id[i] < -2147483648LL || id[i] > 2147483647LL) return set_error(IA3_EINVAL, "%s: %s row %d has region id %lld, outside int32", who, what, i, id[i]);
    ids32[(size_t)i] = (int)id[i];
  }
  std::vector<int> count;
  std::vector<int> sorted;
  for (int c = 0; c < C; ++c) {
    const int lo = start[c], m = start[c + 1] - lo;
    long long mn = ids32[(size_t)lo], mx = mn;
    for (int i = lo; i < lo + m; ++i) { mn = ids32[(size_t)i] < mn ? ids32[(size_t)i] : mn; mx = ids32[(size_t)i] > mx ? ids32[(size_t)i] : mx; }
    int most = 0;
    if (mx - mn < 4LL * m + 1024) {
      count.assign((size_t)(mx - mn + 1), 0);
      for (int i = lo; i < lo + m; ++i) { const int k = ++count[(size_t)(ids32[(size_t)i] - mn)]; most = k > most ? k : most; }
    } else {
      sorted.assign(ids32.begin() + lo, ids32.begin() + lo + m);
      std::sort(sorted.begin(), sorted.end());
      for (int i = 0, run = 0; i < m; ++i) { run = (i && sorted[(size_t)i] == sorted[(size_t)i - 1]) ? run + 1 : 1; most = run > most ? run : most; }
    }
    if (most > IA3_SCORE_MAX_PER_REGION)
      return set_error(IA3_EINVAL, "%s: chromosome %d has %d %s rows of one region id (at most %d are built)", who, c, most, what, IA3_SCORE_MAX_PER_REGION);
  }
  return IA3_OK;
}

// uploads a table and builds its index
int upload_table(const char* who, DevTable& t, const double* rows, const std::vector<int>& ids32, const int* start, int C) {
  t.release();
  const int n = start[C];
  int rc;
  if ((rc = dev_alloc(&t.rows, (size_t)n * 4, who)) || (rc = dev_alloc(&t.id, (size_t)n, who)) || (rc = dev_alloc(&t.start, (size_t)C + 1, who)) ||
      (rc = dev_alloc(&t.sid, (size_t)n, who)) || (rc = dev_alloc(&t.perm, (size_t)n, who))) { t.release(); return rc; }
  t.n = n;
  t.h_start.assign(start, start + C + 1);
  hipStream_t st = stream();
  IA3_HIP(hipMemcpyAsync(t.rows, rows, (size_t)n * 4 * sizeof(double), hipMemcpyHostToDevice, st));
  IA3_HIP(hipMemcpyAsync(t.id, ids32.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, st));
  IA3_HIP(hipMemcpyAsync(t.start, start, ((size_t)C + 1) * sizeof(int), hipMemcpyHostToDevice, st));
  size_t tmp_bytes = 0;
  u64* nokey = nullptr;
  int* norow = nullptr;
  IA3_HIP(rocprim::radix_sort_pairs(nullptr, tmp_bytes, nokey, nokey, norow, norow, (size_t)n, 0, 64, st));
  Scratch k_in((size_t)n * sizeof(u64)), k_out((size_t)n * sizeof(u64)), r_in((size_t)n * sizeof(int)), tmp(tmp_bytes ? tmp_bytes : 8);
  if (!k_in.p || !k_out.p || !r_in.p || !tmp.p) return set_error(IA3_ENOMEM, "%s: scratch to index %d rows", who, n);
  {
    ProfScope ps("score_index");
    hipLaunchKernelGGL(keys_k, dim3(blocks(n, SC_BLOCK)), dim3(SC_BLOCK), 0, st, t.id, t.start, C, n, k_in.as<u64>(), r_in.as<int>());
    IA3_KCHECK();
    IA3_HIP(rocprim::radix_sort_pairs(tmp.p, tmp_bytes, k_in.as<u64>(), k_out.as<u64>(), r_in.as<int>(), t.perm, (size_t)n, 0, 64, st));
    hipLaunchKernelGGL(unkey_k, dim3(blocks(n, SC_BLOCK)), dim3(SC_BLOCK), 0, st, k_out.as<u64>(), n, t.sid);
    IA3_KCHECK();
  }
  IA3_HIP(hipStreamSynchronize(st));   // the host arrays and the scratch may go
  return IA3_OK;
}

}  // namespace

struct ia3_score_population {
  int C = 0;
  DevTable cand, sel;
  double *center_px = nullptr, *dzxy = nullptr, *selmean = nullptr, *center = nullptr;
  int* has_center = nullptr;
  void release() {
    cand.release(); sel.release();
    for (void* p : {(void*)center_px, (void*)dzxy, (void*)selmean, (void*)center, (void*)has_center}) if (p) (void)hipFree(p);
  }
};

namespace {

ScArgs base_args(const ia3_score_population* h, bool on_selected) {
  ScArgs A;
  memset(&A, 0, sizeof(A));
  A.sel = h->sel.view();
  A.tgt = on_selected ? h->sel.view() : h->cand.view();
  A.C = h->C; A.dzxy = h->dzxy; A.center_px = h->center_px; A.has_center = h->has_center;
  A.selmean = h->selmean; A.center = h->center;
  A.step = 1; A.invalid = sc_nan();
  return A;
}

int launch_centers(const ia3_score_population* h) {
  ScArgs A = base_args(h, true);
  hipLaunchKernelGGL(center_k, dim3(blocks(h->C, SC_WAVE)), dim3(SC_WAVE), 0, stream(), A);
  IA3_KCHECK();
  return IA3_OK;
}

// the reference arrays of every chromosome from its selected rows: geom_k on them, then ref_k.  d_* are of 4 S / 4 C values
int run_refs(const ia3_score_population* h, int metric, int half, double intensity_th, int ignore_nan, double* d_raw, double* d_comp,
             double* d_sorted, int* d_counts, int* d_m, double* d_scalars) {
  hipStream_t st = stream();
  const int S = h->sel.n;
  ScArgs A = base_args(h, true);
  A.half = half; A.intensity_th = intensity_th;
  Scratch geom((size_t)5 * S * sizeof(double));
  if (!geom.p) return set_error(IA3_ENOMEM, "score_refs: scratch for %d selected rows", S);
  A.geom = geom.as<double>();
  A.inten = d_raw + (size_t)3 * S;
  ProfScope ps("score_refs");
  hipLaunchKernelGGL(geom_k, dim3(blocks(S, SC_BLOCK)), dim3(SC_BLOCK), 0, st, A);
  IA3_KCHECK();
  // ct, lc and the forward neighbour distance are rows 0, 1 and 2 of geom
  IA3_HIP(hipMemcpyAsync(d_raw, geom.p, (size_t)3 * S * sizeof(double), hipMemcpyDeviceToDevice, st));
  RefArgs R;
  memset(&R, 0, sizeof(R));
  R.C = h->C; R.n_arr = 4; R.stride = S; R.start = h->sel.start; R.raw = d_raw; R.comp = d_comp; R.sorted = d_sorted;
  R.counts = d_counts; R.m = d_m; R.scalars = d_scalars; R.ignore_nan = ignore_nan ? 1 : 0; R.fallback = 1; R.metric = metric;
  R.rows = h->sel.rows; R.dzxy = h->dzxy; R.selmean = h->selmean;
  hipLaunchKernelGGL(ref_k, dim3((unsigned)h->C * 4), dim3(SC_WAVE), 0, st, R);
  IA3_KCHECK();
  return IA3_OK;
}

int check_common(const char* who, const ia3_score_population* h, int half) {
  if (!h) return set_error(IA3_EINVAL, "%s: null population", who);
  if (!h->sel.rows || !h->cand.rows) return set_error(IA3_EINVAL, "%s: the population lost its rows in a failed upload", who);
  if (half < 0 || half > SC_MAX_HALF)
    return set_error(IA3_EINVAL, "%s: a half window of %d regions (0 to %d are built: local_size up to %d)", who, half, SC_MAX_HALF, IA3_SCORE_MAX_LOCAL);
  return IA3_OK;
}

}  // namespace

extern "C" {

int ia3_score_create(const double* cand, const long long* cand_id, const int* cand_start, const double* sel, const long long* sel_id,
                     const int* sel_start, const double* center, const int* has_center, int C, const double* distance_zxy, void** out) {
  if (!out) return set_error(IA3_EINVAL, "score_create: null handle");
  *out = nullptr;
  if (!cand || !cand_id || !cand_start || !sel || !sel_id || !sel_start || !distance_zxy)
    return set_error(IA3_EINVAL, "score_create: null rows, ids, offsets or pixel sizes");
  if (C < 1) return set_error(IA3_EINVAL, "score_create: %d chromosomes", C);
  std::vector<int> cand32, sel32;
  int rc = check_table("score_create", "candidate", cand_id, cand_start, C, cand32); if (rc) return rc;
  rc = check_table("score_create", "selected", sel_id, sel_start, C, sel32); if (rc) return rc;
  rc = ensure_init(); if (rc) return rc;
  ia3_score_population* h = new ia3_score_population();
  h->C = C;
  auto fail = [&](int code) { h->release(); delete h; return code; };
  if ((rc = upload_table("score_create", h->cand, cand, cand32, cand_start, C))) return fail(rc);
  if ((rc = upload_table("score_create", h->sel, sel, sel32, sel_start, C))) return fail(rc);
  if ((rc = dev_alloc(&h->dzxy, 3, "score_create")) || (rc = dev_alloc(&h->selmean, (size_t)3 * C, "score_create")) ||
      (rc = dev_alloc(&h->center, (size_t)3 * C, "score_create"))) return fail(rc);
  hipStream_t st = stream();
  hipError_t e = hipMemcpyAsync(h->dzxy, distance_zxy, 3 * sizeof(double), hipMemcpyHostToDevice, st);
  if (e == hipSuccess && center && has_center) {
    if ((rc = dev_alloc(&h->center_px, (size_t)3 * C, "score_create")) || (rc = dev_alloc(&h->has_center, (size_t)C, "score_create"))) return fail(rc);
    e = hipMemcpyAsync(h->center_px, center, (size_t)3 * C * sizeof(double), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(h->has_center, has_center, (size_t)C * sizeof(int), hipMemcpyHostToDevice, st);
  }
  if (e == hipSuccess && (rc = launch_centers(h))) return fail(rc);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return fail(set_error(IA3_EHIP, "score_create: upload failed: %s", hipGetErrorString(e)));
  *out = h;
  return IA3_OK;
}

int ia3_score_replace_selected(void* handle, const double* sel, const long long* sel_id, const int* sel_start) {
  ia3_score_population* h = (ia3_score_population*)handle;
  if (!h || !sel || !sel_id || !sel_start) return set_error(IA3_EINVAL, "score_replace_selected: null population, rows, ids or offsets");
  std::vector<int> sel32;
  int rc = check_table("score_replace_selected", "selected", sel_id, sel_start, h->C, sel32); if (rc) return rc;
  IA3_HIP(hipStreamSynchronize(stream()));
  rc = upload_table("score_replace_selected", h->sel, sel, sel32, sel_start, h->C); if (rc) return rc;
  rc = launch_centers(h); if (rc) return rc;
  IA3_HIP(hipStreamSynchronize(stream()));
  return IA3_OK;
}

void ia3_score_free(void* handle) {
  ia3_score_population* h = (ia3_score_population*)handle;
  if (!h) return;
  (void)hipStreamSynchronize(stream());
  h->release();
  delete h;
}

int ia3_score_refs_dev(void* handle, int ref_metric, int half, double intensity_th, int ignore_nan, double* arrays, int* counts,
                       double* scalars) {
  ia3_score_population* h = (ia3_score_population*)handle;
  int rc = check_common("score_refs", h, half); if (rc) return rc;
  if (!counts || !scalars) return set_error(IA3_EINVAL, "score_refs: null counts or scalars");
  if (ref_metric < IA3_SCORE_REF_MEDIAN || ref_metric > IA3_SCORE_REF_CDF) return set_error(IA3_EINVAL, "score_refs: reference metric %d", ref_metric);
  const size_t S = (size_t)h->sel.n, C = (size_t)h->C;
  Scratch raw(4 * S * sizeof(double)), comp(4 * S * sizeof(double)), sorted(4 * S * sizeof(double)), cnt(4 * C * sizeof(int)), m(4 * C * sizeof(int)),
      scal(4 * C * sizeof(double));
  if (!raw.p || !comp.p || !sorted.p || !cnt.p || !m.p || !scal.p) return set_error(IA3_ENOMEM, "score_refs: scratch for %zu selected rows", S);
  rc = run_refs(h, ref_metric, half, intensity_th, ignore_nan, raw.as<double>(), comp.as<double>(), sorted.as<double>(), cnt.as<int>(), m.as<int>(),
                scal.as<double>());
  if (rc) return rc;
  hipStream_t st = stream();
  if (arrays) IA3_HIP(hipMemcpyAsync(arrays, comp.p, 4 * S * sizeof(double), hipMemcpyDeviceToHost, st));
  IA3_HIP(hipMemcpyAsync(counts, cnt.p, 4 * C * sizeof(int), hipMemcpyDeviceToHost, st));
  IA3_HIP(hipMemcpyAsync(scalars, scal.p, 4 * C * sizeof(double), hipMemcpyDeviceToHost, st));
  IA3_HIP(hipStreamSynchronize(st));
  return IA3_OK;
}

int ia3_score_scores_dev(void* handle, int kind, int ref_metric, int half, long long step, double invalid, double intensity_th,
                         int ignore_nan, const double* weights, double limit_lo, double limit_hi, double* geom, double* val,
                         unsigned char* cls, int* ref_counts) {
  ia3_score_population* h = (ia3_score_population*)handle;
  int rc = check_common("score_scores", h, half); if (rc) return rc;
  const bool scoring = kind >= 0;
  if (scoring && kind != IA3_SCORE_KIND_DIST_LINEAR && kind != IA3_SCORE_KIND_DIST_CDF) return set_error(IA3_EINVAL, "score_scores: kind %d", kind);
  if (scoring && (!weights || !val || !cls || !ref_counts)) return set_error(IA3_EINVAL, "score_scores: null weights or outputs");
  if (!scoring && !geom) return set_error(IA3_EINVAL, "score_scores: nothing to compute");
  if (scoring && (ref_metric < IA3_SCORE_REF_MEDIAN || ref_metric > IA3_SCORE_REF_CDF || (kind == IA3_SCORE_KIND_DIST_CDF) != (ref_metric == IA3_SCORE_REF_CDF)))
    return set_error(IA3_EINVAL, "score_scores: reference metric %d with kind %d", ref_metric, kind);
  if (step < -2147483647LL || step > 2147483647LL) return set_error(IA3_EINVAL, "score_scores: neighbour step %lld", step);
  const size_t N = (size_t)h->cand.n, S = (size_t)h->sel.n, C = (size_t)h->C;
  hipStream_t st = stream();
  Scratch d_geom(5 * N * sizeof(double));
  if (!d_geom.p) return set_error(IA3_ENOMEM, "score_scores: scratch for %zu candidates", N);
  ScArgs A = base_args(h, false);
  A.half = half; A.step = step; A.invalid = invalid; A.geom = d_geom.as<double>();
  {
    ProfScope ps("score_geom");
    hipLaunchKernelGGL(geom_k, dim3(blocks((long long)N, SC_BLOCK)), dim3(SC_BLOCK), 0, st, A);
    IA3_KCHECK();
  }
  if (geom) IA3_HIP(hipMemcpyAsync(geom, d_geom.p, 5 * N * sizeof(double), hipMemcpyDeviceToHost, st));
  if (!scoring) {
    IA3_HIP(hipStreamSynchronize(st));
    return IA3_OK;
  }
  Scratch raw(4 * S * sizeof(double)), comp(4 * S * sizeof(double)), sorted(4 * S * sizeof(double)), cnt(4 * C * sizeof(int)), m(4 * C * sizeof(int)),
      scal(4 * C * sizeof(double)), d_val(4 * N * sizeof(double)), d_cls(4 * N);
  if (!raw.p || !comp.p || !sorted.p || !cnt.p || !m.p || !scal.p || !d_val.p || !d_cls.p)
    return set_error(IA3_ENOMEM, "score_scores: scratch for %zu candidates and %zu selected rows", N, S);
  rc = run_refs(h, ref_metric, half, intensity_th, ignore_nan, raw.as<double>(), comp.as<double>(), sorted.as<double>(), cnt.as<int>(), m.as<int>(),
                scal.as<double>());
  if (rc) return rc;
  ScoreArgs Q;
  memset(&Q, 0, sizeof(Q));
  Q.C = h->C; Q.N = (int)N; Q.S = (int)S; Q.tgt_start = h->cand.start; Q.ref_start = h->sel.start; Q.n_scores = 4;
  Q.x[0] = d_geom.as<double>(); Q.x[1] = Q.x[0] + N; Q.x[2] = Q.x[0] + 4 * N; Q.x[3] = h->cand.rows; Q.x_stride = 4;
  for (int a = 0; a < 4; ++a) {
    Q.kind[a] = a < 3 ? kind : kind + 2;
    Q.w[a] = weights[a];
    Q.lo[a] = a < 3 ? limit_lo : intensity_th;
    Q.hi[a] = a < 3 ? limit_hi : sc_inf();
  }
  Q.scalars = scal.as<double>(); Q.sorted = sorted.as<double>(); Q.m = m.as<int>(); Q.val = d_val.as<double>(); Q.cls = d_cls.as<unsigned char>();
  {
    ProfScope ps("score_values");
    hipLaunchKernelGGL(score_k, dim3(blocks(4 * (long long)N, SC_BLOCK)), dim3(SC_BLOCK), 0, st, Q);
    IA3_KCHECK();
  }
  IA3_HIP(hipMemcpyAsync(val, d_val.p, 4 * N * sizeof(double), hipMemcpyDeviceToHost, st));
  IA3_HIP(hipMemcpyAsync(cls, d_cls.p, 4 * N, hipMemcpyDeviceToHost, st));
  IA3_HIP(hipMemcpyAsync(ref_counts, m.p, 4 * C * sizeof(int), hipMemcpyDeviceToHost, st));
  IA3_HIP(hipStreamSynchronize(st));
  return IA3_OK;
}

int ia3_score_values_dev(const double* ref_array, int n_ref, double ref_scalar, const double* x, int n, int kind, double weight,
                         double limit_lo, double limit_hi, double* val, unsigned char* cls, int* ref_count) {
  if (!x || !val || !cls || !ref_count) return set_error(IA3_EINVAL, "score_values: null values or outputs");
  if (n < 1) return set_error(IA3_EINVAL, "score_values: %d values", n);
  if (kind < IA3_SCORE_KIND_DIST_LINEAR || kind > IA3_SCORE_KIND_CUM_PROB) return set_error(IA3_EINVAL, "score_values: kind %d", kind);
  const bool cdf = kind == IA3_SCORE_KIND_DIST_CDF || kind == IA3_SCORE_KIND_INT_CDF || kind == IA3_SCORE_KIND_CUM_PROB;
  if (cdf && (!ref_array || n_ref < 1)) return set_error(IA3_EINVAL, "score_values: the cdf kinds need a reference array");
  int rc = ensure_init(); if (rc) return rc;
  hipStream_t st = stream();
  const size_t R = cdf ? (size_t)n_ref : 1;
  Scratch raw(R * sizeof(double)), comp(R * sizeof(double)), sorted(R * sizeof(double)), d_x((size_t)n * sizeof(double)), d_val((size_t)n * sizeof(double)),
      d_cls((size_t)n), small(64);
  if (!raw.p || !comp.p || !sorted.p || !d_x.p || !d_val.p || !d_cls.p || !small.p) return set_error(IA3_ENOMEM, "score_values: scratch for %d values", n);
  // small: start[2], counts, m, then the scalar at byte 32
  int* d_start = small.as<int>();
  double* d_scal = (double*)((char*)small.p + 32);
  const int h_start[4] = {0, cdf ? n_ref : 0, 0, 0};
  IA3_HIP(hipMemcpyAsync(d_start, h_start, sizeof(h_start), hipMemcpyHostToDevice, st));
  IA3_HIP(hipMemcpyAsync(d_scal, &ref_scalar, sizeof(double), hipMemcpyHostToDevice, st));
  IA3_HIP(hipMemcpyAsync(d_x.p, x, (size_t)n * sizeof(double), hipMemcpyHostToDevice, st));
  ProfScope ps("score_values");
  if (cdf) {
    IA3_HIP(hipMemcpyAsync(raw.p, ref_array, R * sizeof(double), hipMemcpyHostToDevice, st));
    RefArgs A;
    memset(&A, 0, sizeof(A));
    A.C = 1; A.n_arr = 1; A.stride = n_ref; A.start = d_start; A.raw = raw.as<double>(); A.comp = comp.as<double>(); A.sorted = sorted.as<double>();
    A.counts = d_start + 2; A.m = d_start + 3; A.scalars = (double*)((char*)small.p + 40); A.ignore_nan = 1; A.fallback = 0; A.metric = SC_REF_CDF;
    hipLaunchKernelGGL(ref_k, dim3(1), dim3(SC_WAVE), 0, st, A);
    IA3_KCHECK();
  }
  ScoreArgs Q;
  memset(&Q, 0, sizeof(Q));
  Q.C = 1; Q.N = n; Q.S = (int)R; Q.tgt_start = nullptr; Q.ref_start = d_start; Q.n_scores = 1; Q.x[0] = d_x.as<double>(); Q.x_stride = 1;
  Q.kind[0] = kind; Q.w[0] = weight; Q.lo[0] = limit_lo; Q.hi[0] = limit_hi;
  Q.scalars = d_scal; Q.sorted = sorted.as<double>(); Q.m = d_start + 3; Q.val = d_val.as<double>(); Q.cls = d_cls.as<unsigned char>();
  hipLaunchKernelGGL(score_k, dim3(blocks(n, SC_BLOCK)), dim3(SC_BLOCK), 0, st, Q);
  IA3_KCHECK();
  IA3_HIP(hipMemcpyAsync(val, d_val.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
  IA3_HIP(hipMemcpyAsync(cls, d_cls.p, (size_t)n, hipMemcpyDeviceToHost, st));
  IA3_HIP(hipMemcpyAsync(ref_count, d_start + 3, sizeof(int), hipMemcpyDeviceToHost, st));
  IA3_HIP(hipStreamSynchronize(st));
  if (!cdf) *ref_count = 0;
  return IA3_OK;
}

int ia3_score_neighbor_lists_dev(void* handle, long long step, double invalid, const int* off_fwd, const int* off_rev, double* fwd,
                                 double* rev) {
  ia3_score_population* h = (ia3_score_population*)handle;
  if (!h || !off_fwd || !off_rev || !fwd || !rev) return set_error(IA3_EINVAL, "score_neighbor_lists: null population, offsets or outputs");
  if (step < -2147483647LL || step > 2147483647LL) return set_error(IA3_EINVAL, "score_neighbor_lists: neighbour step %lld", step);
  const size_t N = (size_t)h->cand.n;
  for (size_t i = 0; i < N; ++i)
    if (off_fwd[i + 1] < off_fwd[i] || off_rev[i + 1] < off_rev[i] || off_fwd[0] != 0 || off_rev[0] != 0)
      return set_error(IA3_EINVAL, "score_neighbor_lists: offsets that do not ascend from 0 at candidate %zu", i);
  const size_t nf = (size_t)off_fwd[N], nr = (size_t)off_rev[N];
  hipStream_t st = stream();
  Scratch d_of((N + 1) * sizeof(int)), d_or((N + 1) * sizeof(int)), d_f((nf ? nf : 1) * sizeof(double)), d_r((nr ? nr : 1) * sizeof(double));
  if (!d_of.p || !d_or.p || !d_f.p || !d_r.p) return set_error(IA3_ENOMEM, "score_neighbor_lists: scratch for %zu distances", nf + nr);
  IA3_HIP(hipMemcpyAsync(d_of.p, off_fwd, (N + 1) * sizeof(int), hipMemcpyHostToDevice, st));
  IA3_HIP(hipMemcpyAsync(d_or.p, off_rev, (N + 1) * sizeof(int), hipMemcpyHostToDevice, st));
  IA3_HIP(hipMemsetAsync(d_f.p, 0xff, (nf ? nf : 1) * sizeof(double), st));   // NaN where the offsets leave more room than values
  IA3_HIP(hipMemsetAsync(d_r.p, 0xff, (nr ? nr : 1) * sizeof(double), st));
  ListArgs L;
  L.A = base_args(h, false);
  L.A.step = step; L.A.invalid = invalid;
  L.off_fwd = d_of.as<int>(); L.off_rev = d_or.as<int>(); L.fwd = d_f.as<double>(); L.rev = d_r.as<double>();
  {
    ProfScope ps("score_lists");
    hipLaunchKernelGGL(lists_k, dim3(blocks((long long)N, SC_BLOCK)), dim3(SC_BLOCK), 0, st, L);
    IA3_KCHECK();
  }
  if (nf) IA3_HIP(hipMemcpyAsync(fwd, d_f.p, nf * sizeof(double), hipMemcpyDeviceToHost, st));
  if (nr) IA3_HIP(hipMemcpyAsync(rev, d_r.p, nr * sizeof(double), hipMemcpyDeviceToHost, st));
  IA3_HIP(hipStreamSynchronize(st));
  return IA3_OK;
}

}  // extern "C"
