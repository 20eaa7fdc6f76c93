// Per-cell spot pickers on the device: spot_tools/picking.py :662-1563 of the reference.
// The candidates of many cells are uploaded once (ia3_cellpick_create) as CSR over cell x region x chromosome, with the
// cells' region ranges, chromosome coordinates and pixel sizes.  The merged lists are made here and stay here.
//   merge_k    one lane per (cell, region): merge_spot_list by the serial text of ia3_cellpick.h
//   naive_k    one lane per (cell, region): the selections of naive_pick_spots_for_chromosomes
//   forward_k  one workgroup of one wavefront per cell, serial over the cell's valid regions in the order the host planned:
//              the K_prev x K_next table of SciPy's cdist distances (select.hip: sqrt((a*a + b*b) + c*c) of the differences
//              in nm) sits in LDS (32 KiB at K = 64), lane c makes chromosome c's allowed indices from its dynamic scores,
//              then lane n picks for spot n of the next region: the measures are recomputed from the distance table per
//              chromosome, the tuples are walked in itertools.product's order and the pointers are stored per (chromosome,
//              merged row) as uint8 (255: none).  The backward pass is the host's, from the downloaded pointers and dynamic scores.
// No floating-point atomics: every value is made by one lane from the inputs alone, so a cell gives the same bits alone
// and inside any batch, on every run.  The one atomic is an integer maximum on a cell's error code.
#include "ia3_rt.h"
#include "ia3_cellpick.h"
#include <math.h>
#include <string.h>
#include <vector>

using namespace ia3rt;
using namespace ia3cp;

namespace {

constexpr int CP_BLOCK = 64;

template <class T>
int dev_alloc(T** p, size_t n, const char* who) {
  *p = nullptr;
  hipError_t e = hipMalloc((void**)p, (n ? n : 1) * sizeof(T));
  if (e != hipSuccess) { *p = nullptr; return set_error(IA3_ENOMEM, "%s: hipMalloc of %zu bytes: %s", who, n * sizeof(T), hipGetErrorString(e)); }
  return IA3_OK;
}

inline unsigned blocks(long long n, int per) { return (unsigned)((n + per - 1) / per); }

struct Dev {
  const double* rows;
  const unsigned char* row_nan;
  const int* cand_start;     // (G * CP_MAX_CHROM + 1)
  const int* region_cell;    // (G)
  const int* n_chrom;        // (n_cells)
  const double* coords;      // (n_cells, CP_MAX_CHROM, 3)
  const int* has_coords;     // (n_cells)
  const int* cap_start;      // (G + 1)
  const double* dzxy;        // 3
  double* merged;            // (cap, 4)
  int* msrc;                 // (cap)
  int* mcount;               // (G)
  int* mvalid;               // (G)
  unsigned char* keep;       // (cap)
  int G;
};

struct MergeArgs {
  Dev D;
  int has_th, hard;
  double th, dist_th;
};

__global__ __launch_bounds__(CP_BLOCK) void merge_k(MergeArgs A) {
  const int g = blockIdx.x * CP_BLOCK + threadIdx.x;
  if (g >= A.D.G) return;
  const int cell = A.D.region_cell[g];
  MergeList L;
  L.rows = A.D.rows;
  L.start = A.D.cand_start + (size_t)g * CP_MAX_CHROM;
  L.coords = A.D.has_coords[cell] ? A.D.coords + (size_t)cell * CP_MAX_CHROM * 3 : nullptr;
  L.C = A.D.n_chrom[cell];
  const size_t at = (size_t)A.D.cap_start[g];
  int valid = 0;
  A.D.mcount[g] = cp_merge_region(L, A.D.row_nan, A.has_th, A.th, A.hard, A.dist_th, A.D.keep + at, A.D.msrc + at, A.D.merged + 4 * at, &valid);
  A.D.mvalid[g] = valid;
}

__global__ __launch_bounds__(CP_BLOCK) void naive_k(Dev D, int mode, int* pick, int* sub) {
  const int g = blockIdx.x * CP_BLOCK + threadIdx.x;
  if (g >= D.G) return;
  const int cell = D.region_cell[g];
  int p[CP_MAX_CHROM], s[CP_MAX_CHROM];
  const int C = D.n_chrom[cell];
  if (mode == CP_NAIVE_MERGED && !D.has_coords[cell]) {   // no coordinate to be near to: nothing is picked
    for (int c = 0; c < CP_MAX_CHROM; ++c) { pick[(size_t)g * CP_MAX_CHROM + c] = -1; sub[(size_t)g * CP_MAX_CHROM + c] = -1; }
    return;
  }
  cp_naive_region(mode, D.rows, D.cand_start + (size_t)g * CP_MAX_CHROM, D.merged + 4 * (size_t)D.cap_start[g], D.mcount[g],
                  D.coords + (size_t)cell * CP_MAX_CHROM * 3, D.dzxy, C, p, s);
  for (int c = 0; c < CP_MAX_CHROM; ++c) {
    pick[(size_t)g * CP_MAX_CHROM + c] = c < C ? p[c] : -1;
    sub[(size_t)g * CP_MAX_CHROM + c] = c < C ? s[c] : -1;
  }
}

struct FwdArgs {
  Dev D;
  const int* cells;
  const int* vstart;
  const int* vreg;
  const long long* vgap;
  double* dy;            // (largest n_chrom, stride)
  unsigned char* ptr;    // (largest n_chrom, stride), 255: none
  size_t stride;
  int kind;
  const double* ref_scalar;
  const int* ref_start;
  const double* sorted;
  const double* table;
  double w, hi, nan_mask;
  int share;
  int* err;
};

__global__ __launch_bounds__(CP_BLOCK) void forward_k(FwdArgs A) {
  __shared__ double dist[CP_MAX_SPOTS * CP_MAX_SPOTS];
  __shared__ int allowed[CP_MAX_CHROM][CP_MAX_SPOTS];
  __shared__ int na[CP_MAX_CHROM];
  const int cell = A.cells[blockIdx.x], lane = threadIdx.x;
  const int C = A.D.n_chrom[cell];
  NbRef refs[CP_MAX_CHROM];
  for (int c = 0; c < CP_MAX_CHROM; ++c) {
    const int j = cell * CP_MAX_CHROM + c;
    NbRef& r = refs[c];
    r.kind = A.kind; r.w = A.w; r.hi = A.hi; r.nan_mask = A.nan_mask;
    r.ref = A.ref_scalar ? A.ref_scalar[j] : 0.0;
    r.sorted = nullptr; r.table = nullptr; r.n = 0;
    if (A.kind == ia3sc::SC_DIST_CDF && c < C) {
      r.sorted = A.sorted + A.ref_start[j];
      r.table = A.table + A.ref_start[j] + j;
      r.n = A.ref_start[j + 1] - A.ref_start[j];
    }
  }
  const double dz = A.D.dzxy[0], dx = A.D.dzxy[1], dyy = A.D.dzxy[2];
  for (int s = A.vstart[cell]; s + 1 < A.vstart[cell + 1]; ++s) {
    const int g0 = A.vreg[s], g1 = A.vreg[s + 1];
    const int K0 = A.D.mcount[g0], K1 = A.D.mcount[g1];
    const size_t b0 = (size_t)A.D.cap_start[g0], b1 = (size_t)A.D.cap_start[g1];
    const long long gap = A.vgap[s + 1];
    if (lane < K1) {
      const double* m = A.D.merged + 4 * (b1 + lane);
      const double z = m[1] * dz, x = m[2] * dx, y = m[3] * dyy;
      for (int p = 0; p < K0; ++p) {
        const double* q = A.D.merged + 4 * (b0 + p);
        dist[p * CP_MAX_SPOTS + lane] = ia3sc::sc_norm_rows(q[1] * dz - z, q[2] * dx - x, q[3] * dyy - y);
      }
    }
    if (lane < C) {
      const double* d = A.dy + (size_t)lane * A.stride + b0;
      na[lane] = cp_allowed([&](int p) { return d[p]; }, K0, C, allowed[lane]);
    }
    __syncthreads();
    if (lane < K1) {
      auto meas = [&](int c, int p) { return cp_measure(refs[c], dist[p * CP_MAX_SPOTS + lane], gap, A.dy[(size_t)c * A.stride + b0 + p]); };
      int sel[CP_MAX_CHROM];
      const int rc = cp_pick(C, K0, na, [&](int c, int a) { return allowed[c][a]; }, meas, A.share != 0, sel);
      if (rc != CP_OK) {
        atomicMax(A.err + cell, rc);
      } else {
        for (int c = 0; c < C; ++c) {
          const size_t at = (size_t)c * A.stride + b1 + lane;
          A.dy[at] += meas(c, sel[c]);
          A.ptr[at] = (unsigned char)sel[c];
        }
      }
    }
    __syncthreads();
  }
}

}  // namespace

struct ia3_cellpick_population {
  int n_cells = 0, G = 0, planes = 1;   // planes: the largest n_chrom
  size_t n = 0, cap = 0;
  double *rows = nullptr, *coords = nullptr, *dzxy = nullptr, *merged = nullptr;
  unsigned char *row_nan = nullptr, *keep = nullptr;
  int *cand_start = nullptr, *region_cell = nullptr, *n_chrom = nullptr, *has_coords = nullptr, *cap_start = nullptr, *msrc = nullptr,
      *mcount = nullptr, *mvalid = nullptr, *vstart = nullptr, *vreg = nullptr;
  long long* vgap = nullptr;
  std::vector<int> h_region_start, h_n_chrom, h_has_coords, h_cap_start, h_mcount, h_vstart;
  bool merged_done = false, planned = false;
  void release() {
    for (void* p : {(void*)rows, (void*)coords, (void*)dzxy, (void*)merged, (void*)row_nan, (void*)keep, (void*)cand_start, (void*)region_cell,
                    (void*)n_chrom, (void*)has_coords, (void*)cap_start, (void*)msrc, (void*)mcount, (void*)mvalid, (void*)vstart, (void*)vreg,
                    (void*)vgap})
      if (p) (void)hipFree(p);
  }
  Dev view() const {
    Dev D;
    D.rows = rows; D.row_nan = row_nan; D.cand_start = cand_start; D.region_cell = region_cell; D.n_chrom = n_chrom; D.coords = coords;
    D.has_coords = has_coords; D.cap_start = cap_start; D.dzxy = dzxy; D.merged = merged; D.msrc = msrc; D.mcount = mcount; D.mvalid = mvalid;
    D.keep = keep; D.G = G;
    return D;
  }
};

extern "C" {

int ia3_cellpick_create(const double* rows, const unsigned char* row_nan, const int* cand_start, const int* region_start,
                        const int* n_chrom, const double* coords, const int* has_coords, const int* cap_start, int n_cells,
                        int G, const double* distance_zxy, void** out) {
  const char* who = "cellpick_create";
  if (!out) return set_error(IA3_EINVAL, "%s: null handle", who);
  *out = nullptr;
  if (!rows || !row_nan || !cand_start || !region_start || !n_chrom || !coords || !has_coords || !cap_start || !distance_zxy)
    return set_error(IA3_EINVAL, "%s: null rows, offsets, chromosomes, coordinates or pixel sizes", who);
  if (n_cells < 1 || G < 1 || (long long)G * CP_MAX_CHROM + 1 > 2147483647LL) return set_error(IA3_EINVAL, "%s: %d cells with %d regions", who, n_cells, G);
  if (region_start[0] != 0 || region_start[n_cells] != G) return set_error(IA3_EINVAL, "%s: the region offsets run from %d to %d for %d regions", who, region_start[0], region_start[n_cells], G);
  std::vector<int> region_cell((size_t)G);
  for (int k = 0; k < n_cells; ++k) {
    if (region_start[k + 1] < region_start[k]) return set_error(IA3_EINVAL, "%s: the region offsets descend at cell %d", who, k);
    if (n_chrom[k] < 1 || n_chrom[k] > CP_MAX_CHROM)
      return set_error(IA3_EINVAL, "%s: cell %d has %d chromosomes (1 to %d are built)", who, k, n_chrom[k], CP_MAX_CHROM);
    for (int g = region_start[k]; g < region_start[k + 1]; ++g) region_cell[g] = k;
  }
  int planes = 1;
  for (int k = 0; k < n_cells; ++k) planes = n_chrom[k] > planes ? n_chrom[k] : planes;
  const size_t S = (size_t)G * CP_MAX_CHROM;
  if (cand_start[0] != 0 || cap_start[0] != 0) return set_error(IA3_EINVAL, "%s: offsets that do not start at 0", who);
  for (size_t i = 0; i < S; ++i)
    if (cand_start[i + 1] < cand_start[i]) return set_error(IA3_EINVAL, "%s: the candidate offsets descend at slot %zu", who, i);
  for (int g = 0; g < G; ++g) {
    const int C = n_chrom[region_cell[g]];
    const size_t s = (size_t)g * CP_MAX_CHROM;
    if (cand_start[s + CP_MAX_CHROM] != cand_start[s + C]) return set_error(IA3_EINVAL, "%s: region %d has candidates beyond its %d chromosomes", who, g, C);
    const long long need = (long long)(cand_start[s + C] - cand_start[s]) + 2 * C;
    if ((long long)cap_start[g + 1] - cap_start[g] < need) return set_error(IA3_EINVAL, "%s: region %d has room for %d merged rows, %lld may come", who, g, cap_start[g + 1] - cap_start[g], need);
  }
  int rc = ensure_init(); if (rc) return rc;
  ia3_cellpick_population* h = new ia3_cellpick_population();
  h->n_cells = n_cells; h->G = G; h->planes = planes; h->n = (size_t)cand_start[S]; h->cap = (size_t)cap_start[G];
  h->h_region_start.assign(region_start, region_start + n_cells + 1);
  h->h_n_chrom.assign(n_chrom, n_chrom + n_cells);
  h->h_has_coords.assign(has_coords, has_coords + n_cells);
  h->h_cap_start.assign(cap_start, cap_start + G + 1);
  auto fail = [&](int code) { h->release(); delete h; return code; };
  const size_t NC = (size_t)n_cells;
  if ((rc = dev_alloc(&h->rows, h->n * 4, who)) || (rc = dev_alloc(&h->row_nan, h->n, who)) || (rc = dev_alloc(&h->cand_start, S + 1, who)) ||
      (rc = dev_alloc(&h->region_cell, (size_t)G, who)) || (rc = dev_alloc(&h->n_chrom, NC, who)) || (rc = dev_alloc(&h->coords, NC * CP_MAX_CHROM * 3, who)) ||
      (rc = dev_alloc(&h->has_coords, NC, who)) || (rc = dev_alloc(&h->cap_start, (size_t)G + 1, who)) || (rc = dev_alloc(&h->dzxy, 3, who)) ||
      (rc = dev_alloc(&h->merged, h->cap * 4, who)) || (rc = dev_alloc(&h->msrc, h->cap, who)) || (rc = dev_alloc(&h->keep, h->cap, who)) ||
      (rc = dev_alloc(&h->mcount, (size_t)G, who)) || (rc = dev_alloc(&h->mvalid, (size_t)G, who)))
    return fail(rc);
  hipStream_t st = stream();
  hipError_t e = hipSuccess;
  auto up = [&](void* d, const void* s, size_t bytes) { if (e == hipSuccess && bytes) e = hipMemcpyAsync(d, s, bytes, hipMemcpyHostToDevice, st); };
  up(h->rows, rows, h->n * 4 * sizeof(double));
  up(h->row_nan, row_nan, h->n);
  up(h->cand_start, cand_start, (S + 1) * sizeof(int));
  up(h->region_cell, region_cell.data(), (size_t)G * sizeof(int));
  up(h->n_chrom, n_chrom, NC * sizeof(int));
  up(h->coords, coords, NC * CP_MAX_CHROM * 3 * sizeof(double));
  up(h->has_coords, has_coords, NC * sizeof(int));
  up(h->cap_start, cap_start, ((size_t)G + 1) * sizeof(int));
  up(h->dzxy, distance_zxy, 3 * sizeof(double));
  if (e == hipSuccess) e = hipStreamSynchronize(st);    // region_cell is a local
  if (e != hipSuccess) return fail(set_error(IA3_EHIP, "%s: upload failed: %s", who, hipGetErrorString(e)));
  *out = h;
  return IA3_OK;
}

void ia3_cellpick_free(void* handle) {
  ia3_cellpick_population* h = (ia3_cellpick_population*)handle;
  if (!h) return;
  (void)hipStreamSynchronize(stream());
  h->release();
  delete h;
}

int ia3_cellpick_merge_dev(void* handle, int has_th, double intensity_th, int hard, double dist_th, int* count, int* valid, int* src) {
  ia3_cellpick_population* h = (ia3_cellpick_population*)handle;
  if (!h || !count || !valid || !src) return set_error(IA3_EINVAL, "cellpick_merge: null population or outputs");
  hipStream_t st = stream();
  MergeArgs A;
  A.D = h->view(); A.has_th = has_th ? 1 : 0; A.hard = hard ? 1 : 0; A.th = intensity_th; A.dist_th = dist_th;
  h->merged_done = false; h->planned = false;
  IA3_HIP(hipMemsetAsync(h->msrc, 0, h->cap * sizeof(int), st));
  IA3_HIP(hipMemsetAsync(h->merged, 0, h->cap * 4 * sizeof(double), st));
  {
    ProfScope ps("cellpick_merge");
    hipLaunchKernelGGL(merge_k, dim3(blocks(h->G, CP_BLOCK)), dim3(CP_BLOCK), 0, st, A);
    IA3_KCHECK();
  }
  IA3_HIP(hipMemcpyAsync(count, h->mcount, (size_t)h->G * sizeof(int), hipMemcpyDeviceToHost, st));
  IA3_HIP(hipMemcpyAsync(valid, h->mvalid, (size_t)h->G * sizeof(int), hipMemcpyDeviceToHost, st));
  IA3_HIP(hipMemcpyAsync(src, h->msrc, h->cap * sizeof(int), hipMemcpyDeviceToHost, st));
  IA3_HIP(hipStreamSynchronize(st));
  h->h_mcount.assign(count, count + h->G);
  h->merged_done = true;
  return IA3_OK;
}

int ia3_cellpick_naive_dev(void* handle, int mode, int* pick, int* sub) {
  ia3_cellpick_population* h = (ia3_cellpick_population*)handle;
  if (!h || !pick || !sub) return set_error(IA3_EINVAL, "cellpick_naive: null population or outputs");
  if (mode != IA3_CELLPICK_NAIVE_OWN && mode != IA3_CELLPICK_NAIVE_MERGED) return set_error(IA3_EINVAL, "cellpick_naive: mode %d", mode);
  if (mode == IA3_CELLPICK_NAIVE_MERGED && !h->merged_done) return set_error(IA3_EINVAL, "cellpick_naive: the lists are not merged");
  hipStream_t st = stream();
  const size_t S = (size_t)h->G * CP_MAX_CHROM;
  Scratch d_pick(S * sizeof(int)), d_sub(S * sizeof(int));
  if (!d_pick.p || !d_sub.p) return set_error(IA3_ENOMEM, "cellpick_naive: scratch for %d regions", h->G);
  {
    ProfScope ps("cellpick_naive");
    hipLaunchKernelGGL(naive_k, dim3(blocks(h->G, CP_BLOCK)), dim3(CP_BLOCK), 0, st, h->view(), mode, d_pick.as<int>(), d_sub.as<int>());
    IA3_KCHECK();
  }
  IA3_HIP(hipMemcpyAsync(pick, d_pick.p, S * sizeof(int), hipMemcpyDeviceToHost, st));
  IA3_HIP(hipMemcpyAsync(sub, d_sub.p, S * sizeof(int), hipMemcpyDeviceToHost, st));
  IA3_HIP(hipStreamSynchronize(st));
  return IA3_OK;
}

int ia3_cellpick_plan(void* handle, const int* vstart, const int* vreg, const long long* vgap) {
  ia3_cellpick_population* h = (ia3_cellpick_population*)handle;
  if (!h || !vstart || !vreg || !vgap) return set_error(IA3_EINVAL, "cellpick_plan: null population or lists");
  if (!h->merged_done) return set_error(IA3_EINVAL, "cellpick_plan: the lists are not merged");
  if (vstart[0] != 0) return set_error(IA3_EINVAL, "cellpick_plan: the offsets start at %d", vstart[0]);
  for (int k = 0; k < h->n_cells; ++k) {
    if (vstart[k + 1] < vstart[k] || vstart[k + 1] - vstart[k] > h->h_region_start[k + 1] - h->h_region_start[k])
      return set_error(IA3_EINVAL, "cellpick_plan: cell %d walks %d of its %d regions", k, vstart[k + 1] - vstart[k], h->h_region_start[k + 1] - h->h_region_start[k]);
    for (int s = vstart[k]; s < vstart[k + 1]; ++s) {
      const int g = vreg[s];
      if (g < h->h_region_start[k] || g >= h->h_region_start[k + 1]) return set_error(IA3_EINVAL, "cellpick_plan: region %d is not one of cell %d", g, k);
      if (h->h_mcount[g] < 1 || h->h_mcount[g] > CP_MAX_SPOTS || h->h_mcount[g] > h->h_cap_start[g + 1] - h->h_cap_start[g])
        return set_error(IA3_EUNSUPPORTED, "cellpick_plan: region %d has %d merged spots (1 to %d are built)", g, h->h_mcount[g], CP_MAX_SPOTS);
    }
  }
  hipStream_t st = stream();
  IA3_HIP(hipStreamSynchronize(st));
  h->planned = false;
  for (void* p : {(void*)h->vstart, (void*)h->vreg, (void*)h->vgap}) if (p) (void)hipFree(p);
  h->vstart = nullptr; h->vreg = nullptr; h->vgap = nullptr;
  const size_t nv = (size_t)vstart[h->n_cells];
  int rc;
  if ((rc = dev_alloc(&h->vstart, (size_t)h->n_cells + 1, "cellpick_plan")) || (rc = dev_alloc(&h->vreg, nv, "cellpick_plan")) ||
      (rc = dev_alloc(&h->vgap, nv, "cellpick_plan"))) return rc;
  IA3_HIP(hipMemcpyAsync(h->vstart, vstart, ((size_t)h->n_cells + 1) * sizeof(int), hipMemcpyHostToDevice, st));
  if (nv) IA3_HIP(hipMemcpyAsync(h->vreg, vreg, nv * sizeof(int), hipMemcpyHostToDevice, st));
  if (nv) IA3_HIP(hipMemcpyAsync(h->vgap, vgap, nv * sizeof(long long), hipMemcpyHostToDevice, st));
  IA3_HIP(hipStreamSynchronize(st));
  h->h_vstart.assign(vstart, vstart + h->n_cells + 1);
  h->planned = true;
  return IA3_OK;
}

int ia3_cellpick_forward_dev(void* handle, const int* cells, int n_active, const double* scores, int kind, const double* ref_scalar,
                             const int* ref_start, const double* sorted, const double* table, double weight, double limit_hi,
                             double nan_mask, int share, double* dy, unsigned char* ptr, int* err) {
  const char* who = "cellpick_forward";
  ia3_cellpick_population* h = (ia3_cellpick_population*)handle;
  if (!h || !cells || !scores || !dy || !ptr || !err) return set_error(IA3_EINVAL, "%s: null population, cells, scores or outputs", who);
  if (!h->planned) return set_error(IA3_EINVAL, "%s: the walk is not planned", who);
  if (n_active < 1 || n_active > h->n_cells) return set_error(IA3_EINVAL, "%s: %d of %d cells", who, n_active, h->n_cells);
  for (int i = 0; i < n_active; ++i)
    if (cells[i] < 0 || cells[i] >= h->n_cells || (i && cells[i] <= cells[i - 1])) return set_error(IA3_EINVAL, "%s: the cells do not ascend within 0 .. %d", who, h->n_cells - 1);
  const bool cdf = kind == IA3_SCORE_KIND_DIST_CDF;
  if (!cdf && kind != IA3_SCORE_KIND_DIST_LINEAR) return set_error(IA3_EINVAL, "%s: kind %d", who, kind);
  const size_t J = (size_t)h->n_cells * CP_MAX_CHROM;
  size_t n_ref = 0;
  if (cdf) {
    if (!ref_start || !sorted || !table) return set_error(IA3_EINVAL, "%s: the cdf kind needs reference arrays and tables", who);
    if (ref_start[0] != 0) return set_error(IA3_EINVAL, "%s: the reference offsets start at %d", who, ref_start[0]);
    for (size_t j = 0; j < J; ++j)
      if (ref_start[j + 1] < ref_start[j]) return set_error(IA3_EINVAL, "%s: the reference offsets descend at %zu", who, j);
    for (int i = 0; i < n_active && weight != 0.0; ++i)
      for (int c = 0; c < h->h_n_chrom[cells[i]]; ++c) {
        const size_t j = (size_t)cells[i] * CP_MAX_CHROM + c;
        if (ref_start[j + 1] - ref_start[j] < 1) return set_error(IA3_EINVAL, "%s: chromosome %d of cell %d has no reference value", who, c, cells[i]);
      }
    n_ref = (size_t)ref_start[J];
  } else if (!ref_scalar) {
    return set_error(IA3_EINVAL, "%s: the linear kind needs reference distances", who);
  }
  hipStream_t st = stream();
  const size_t T = (size_t)h->planes * h->cap;
  Scratch d_cells((size_t)n_active * sizeof(int)), d_dy(T * sizeof(double)), d_ptr(T), d_err((size_t)h->n_cells * sizeof(int)), d_scal(J * sizeof(double)),
      d_rs((J + 1) * sizeof(int)), d_sorted((n_ref ? n_ref : 1) * sizeof(double)), d_table((n_ref + J + 1) * sizeof(double));
  if (!d_cells.p || !d_dy.p || !d_ptr.p || !d_err.p || !d_scal.p || !d_rs.p || !d_sorted.p || !d_table.p)
    return set_error(IA3_ENOMEM, "%s: scratch for %zu merged rows", who, h->cap);
  IA3_HIP(hipMemcpyAsync(d_cells.p, cells, (size_t)n_active * sizeof(int), hipMemcpyHostToDevice, st));
  IA3_HIP(hipMemcpyAsync(d_dy.p, scores, T * sizeof(double), hipMemcpyHostToDevice, st));
  IA3_HIP(hipMemsetAsync(d_ptr.p, 0xff, T, st));
  IA3_HIP(hipMemsetAsync(d_err.p, 0, (size_t)h->n_cells * sizeof(int), st));
  if (cdf) {
    IA3_HIP(hipMemcpyAsync(d_rs.p, ref_start, (J + 1) * sizeof(int), hipMemcpyHostToDevice, st));
    if (n_ref) IA3_HIP(hipMemcpyAsync(d_sorted.p, sorted, n_ref * sizeof(double), hipMemcpyHostToDevice, st));
    IA3_HIP(hipMemcpyAsync(d_table.p, table, (n_ref + J) * sizeof(double), hipMemcpyHostToDevice, st));
  } else {
    IA3_HIP(hipMemcpyAsync(d_scal.p, ref_scalar, J * sizeof(double), hipMemcpyHostToDevice, st));
  }
  FwdArgs A;
  A.D = h->view(); A.cells = d_cells.as<int>(); A.vstart = h->vstart; A.vreg = h->vreg; A.vgap = h->vgap;
  A.dy = d_dy.as<double>(); A.ptr = d_ptr.as<unsigned char>(); A.stride = h->cap; A.kind = kind;
  A.ref_scalar = cdf ? nullptr : d_scal.as<double>(); A.ref_start = d_rs.as<int>(); A.sorted = d_sorted.as<double>(); A.table = d_table.as<double>();
  A.w = weight; A.hi = limit_hi; A.nan_mask = nan_mask; A.share = share ? 1 : 0; A.err = d_err.as<int>();
  {
    ProfScope ps("cellpick_forward");
    hipLaunchKernelGGL(forward_k, dim3((unsigned)n_active), dim3(CP_BLOCK), 0, st, A);
    IA3_KCHECK();
  }
  IA3_HIP(hipMemcpyAsync(dy, d_dy.p, T * sizeof(double), hipMemcpyDeviceToHost, st));
  IA3_HIP(hipMemcpyAsync(ptr, d_ptr.p, T, hipMemcpyDeviceToHost, st));
  IA3_HIP(hipMemcpyAsync(err, d_err.p, (size_t)h->n_cells * sizeof(int), hipMemcpyDeviceToHost, st));
  IA3_HIP(hipStreamSynchronize(st));
  return IA3_OK;
}

}  // extern "C"
