// A/B compartment densities of traced cells on the device: compartment_tools/density.py:4-102, the sum of
// Gaussian terms exp(-0.5 * sum((c - q)**2 / sigma**2)) over the A loci and over the B loci of a nucleus for every locus q
// of that nucleus, all pairs per cell.  The loci of all cells are uploaded once (ia3_density_create); a scoring call
// (ia3_density_scores_dev) brings the labels (how often a locus id counts as A and as B), the squared sigmas and the flags.
//   density_k   a workgroup owns DN_QTILE consecutive queries of one cell, one per lane (the host's work list names the
//               cell and the first query).  The cell's contributors pass through LDS DN_CTILE at a time, 32 bytes each
//               (z, x, y and one word with the copy and the two multiplicities); every lane reads the same contributor,
//               a broadcast.  A contributor listed under neither key is skipped by the whole workgroup.  A lane keeps two
//               float64 sums and two integer counts; each sum is made of partial sums over DN_PART consecutive
//               contributors that are then added in order, which is what the tolerance of the tests is derived from.
// LDS: 8 KiB per workgroup of two waves.  No atomics, no dependence on the launch shape: the same bits on every run and
// for every set of other cells in the population.
#include "ia3_rt.h"
#include "ia3_density.h"
#include <math.h>
#include <string.h>
#include <vector>

using namespace ia3rt;
using namespace ia3dn;

namespace {

struct alignas(16) DnStage { double z, x, y; uint32_t word, pad; };
static_assert(sizeof(DnStage) == 32, "two 16-byte reads per contributor");

struct DnArgs {
  const double* z; const double* x; const double* y;   // n_points each
  const int* copy; const int* locus;                   // locus: n_loci for a point that is not finite
  const unsigned char* mult;                           // (n_loci + 1) x 2, the last pair 0
  const int* cell_start;
  const int2* work;                                    // (cell, first query)
  double s2z, s2x, s2y;
  int flags;
  long long n_points;
  double* sums; int* counts;
};

__device__ inline double qnan() { return __longlong_as_double(0x7ff8000000000000LL); }

__global__ __launch_bounds__(DN_QTILE) void density_k(DnArgs A) {
  __shared__ DnStage s[DN_CTILE];
  const int2 w = A.work[blockIdx.x];
  const int c0 = A.cell_start[w.x], c1 = A.cell_start[w.x + 1];
  const int q = w.y + (int)threadIdx.x;
  const bool live = q < c1;
  const double qz = live ? A.z[q] : 0.0, qx = live ? A.x[q] : 0.0, qy = live ? A.y[q] : 0.0;
  const int qc = live ? A.copy[q] : -1;
  const int flags = live ? A.flags : 0;   // a lane without a query weighs nothing
  double acc_a = 0.0, acc_b = 0.0;
  int n_a = 0, n_b = 0;
  for (int j0 = c0; j0 < c1; j0 += DN_CTILE) {
    const int cnt = min(DN_CTILE, c1 - j0);
    for (int i = threadIdx.x; i < cnt; i += DN_QTILE) {
      const int j = j0 + i, id = A.locus[j];
      DnStage t;
      t.z = A.z[j]; t.x = A.x[j]; t.y = A.y[j];
      t.word = dn_pack(A.copy[j], A.mult[2 * id], A.mult[2 * id + 1]);
      t.pad = 0;
      s[i] = t;
    }
    __syncthreads();
    for (int p0 = 0; p0 < cnt; p0 += DN_PART) {
      const int p1 = min(cnt, p0 + DN_PART);
      double part_a = 0.0, part_b = 0.0;
      for (int i = p0; i < p1; ++i) {
        const uint32_t word = s[i].word;
        if ((word >> 16) == 0) continue;   // listed under neither key, or not finite: the same for every lane
        const bool same = dn_copy(word) == qc, self = j0 + i == q;
        const int wa = dn_weight(same, self, dn_mult_a(word), flags), wb = dn_weight(same, self, dn_mult_b(word), flags);
        if (wa | wb) {
          const double t = dn_arg(s[i].z, s[i].x, s[i].y, qz, qx, qy, A.s2z, A.s2x, A.s2y);
          const double e = t < DN_CUT ? 0.0 : exp(t);   // a NaN argument (sigma 0) stays NaN
          if (wa) { part_a += (double)wa * e; n_a += wa; }
          if (wb) { part_b += (double)wb * e; n_b += wb; }
        }
      }
      acc_a += part_a;
      acc_b += part_b;
    }
    __syncthreads();
  }
  if (!live) return;
  const bool nan = qz != qz || qx != qx || qy != qy;   // density.py:35: the query is skipped
  A.sums[q] = nan ? qnan() : acc_a;
  A.sums[A.n_points + q] = nan ? qnan() : acc_b;
  A.counts[q] = n_a;
  A.counts[A.n_points + q] = n_b;
}

}  // namespace

struct ia3_density_population {
  int n_cells = 0, n_loci = 0, n_work = 0;
  long long n_points = 0;
  char* d = nullptr;   // one allocation: z, x, y, copy, locus, cell_start, work, mult
  double* z = nullptr; double* x = nullptr; double* y = nullptr;
  int* copy = nullptr; int* locus = nullptr; int* cell_start = nullptr;
  int2* work = nullptr;
  unsigned char* mult = nullptr;
};

extern "C" {

int ia3_density_create(const double* zxys, const int* cell_start, const int* copy_of, const int* locus_of, int n_cells,
                       int n_loci, void** out) {
  int rc = ensure_init(); if (rc) return rc;
  if (!out) return set_error(IA3_EINVAL, "density_create: null handle");
  *out = nullptr;
  if (n_cells < 1 || n_loci < 1 || !cell_start || cell_start[0] != 0)
    return set_error(IA3_EINVAL, "density_create: %d cells, %d locus ids, or a table that does not start at 0", n_cells, n_loci);
  for (int c = 0; c < n_cells; ++c) {
    const long long size = (long long)cell_start[c + 1] - cell_start[c];
    if (size < 0) return set_error(IA3_EINVAL, "density_create: cell_start falls at cell %d", c);
    if (size > IA3_DENSITY_MAX_CELL) return set_error(IA3_EINVAL, "density_create: cell %d has %lld loci (at most %d)", c, size, IA3_DENSITY_MAX_CELL);
  }
  const long long n = cell_start[n_cells];
  if (n > 0 && (!zxys || !copy_of || !locus_of)) return set_error(IA3_EINVAL, "density_create: null coordinates, copies or locus ids");
  std::vector<int2> work;
  for (int c = 0; c < n_cells; ++c)
    for (int q0 = cell_start[c]; q0 < cell_start[c + 1]; q0 += DN_QTILE) work.push_back(make_int2(c, q0));
  // the host image of the allocation; every block starts on a multiple of 16 bytes
  auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
  const size_t np = (size_t)(n > 0 ? n : 1), nw = work.empty() ? 1 : work.size();
  const size_t o_z = 0, o_x = up16(o_z + np * 8), o_y = up16(o_x + np * 8), o_copy = up16(o_y + np * 8), o_locus = up16(o_copy + np * 4),
               o_start = up16(o_locus + np * 4), o_work = up16(o_start + ((size_t)n_cells + 1) * 4), o_mult = up16(o_work + nw * sizeof(int2)),
               bytes = up16(o_mult + ((size_t)n_loci + 1) * 2);
  std::vector<char> host(bytes, 0);
  double* hz = (double*)(host.data() + o_z); double* hx = (double*)(host.data() + o_x); double* hy = (double*)(host.data() + o_y);
  int* hc = (int*)(host.data() + o_copy); int* hl = (int*)(host.data() + o_locus);
  for (long long p = 0; p < n; ++p) {
    const double vz = zxys[3 * p], vx = zxys[3 * p + 1], vy = zxys[3 * p + 2];
    if (copy_of[p] < 0 || copy_of[p] >= IA3_DENSITY_MAX_CELL || locus_of[p] < 0 || locus_of[p] >= n_loci)
      return set_error(IA3_EINVAL, "density_create: point %lld has copy %d and locus id %d of %d", p, copy_of[p], locus_of[p], n_loci);
    hz[p] = vz; hx[p] = vx; hy[p] = vy;
    hc[p] = copy_of[p];
    hl[p] = (isfinite(vz) && isfinite(vx) && isfinite(vy)) ? locus_of[p] : n_loci;   // the id of weight 0
  }
  memcpy(host.data() + o_start, cell_start, ((size_t)n_cells + 1) * 4);
  if (!work.empty()) memcpy(host.data() + o_work, work.data(), work.size() * sizeof(int2));
  ia3_density_population* h = new ia3_density_population();
  h->n_cells = n_cells; h->n_loci = n_loci; h->n_points = n; h->n_work = (int)work.size();
  hipError_t e = hipMalloc((void**)&h->d, bytes);
  if (e != hipSuccess) { delete h; return set_error(IA3_ENOMEM, "density_create: hipMalloc of %zu bytes: %s", bytes, hipGetErrorString(e)); }
  h->z = (double*)(h->d + o_z); h->x = (double*)(h->d + o_x); h->y = (double*)(h->d + o_y);
  h->copy = (int*)(h->d + o_copy); h->locus = (int*)(h->d + o_locus); h->cell_start = (int*)(h->d + o_start);
  h->work = (int2*)(h->d + o_work); h->mult = (unsigned char*)(h->d + o_mult);
  hipStream_t st = stream();
  e = hipMemcpyAsync(h->d, host.data(), bytes, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) { (void)hipFree(h->d); delete h; return set_error(IA3_EHIP, "density_create: upload failed: %s", hipGetErrorString(e)); }
  *out = h;
  return IA3_OK;
}

void ia3_density_free(void* handle) {
  ia3_density_population* h = (ia3_density_population*)handle;
  if (!h) return;
  (void)hipStreamSynchronize(stream());
  if (h->d) (void)hipFree(h->d);
  delete h;
}

int ia3_density_scores_dev(void* handle, const unsigned char* mult, const double* s2, int use_cis, int use_trans, int exclude_self,
                           double* sums, int* counts) {
  ia3_density_population* h = (ia3_density_population*)handle;
  if (!h || !mult || !s2 || !sums || !counts) return set_error(IA3_EINVAL, "density_scores: null population, labels, sigmas or outputs");
  if (!use_cis && !use_trans) return set_error(IA3_EINVAL, "density_scores: one of use_cis or use_trans is required");
  if (h->n_points == 0) return IA3_OK;
  hipStream_t st = stream();
  const size_t n = (size_t)h->n_points;
  Scratch d_sums(2 * n * sizeof(double)), d_counts(2 * n * sizeof(int));
  if (!d_sums.p || !d_counts.p) return set_error(IA3_ENOMEM, "density_scores: scratch for %zu points", n);
  IA3_HIP(hipMemcpyAsync(h->mult, mult, (size_t)h->n_loci * 2, hipMemcpyHostToDevice, st));   // the pair after them stays 0
  DnArgs A;
  A.z = h->z; A.x = h->x; A.y = h->y; A.copy = h->copy; A.locus = h->locus; A.mult = h->mult;
  A.cell_start = h->cell_start; A.work = h->work;
  A.s2z = s2[0]; A.s2x = s2[1]; A.s2y = s2[2];
  A.flags = (use_cis ? DN_USE_CIS : 0) | (use_trans ? DN_USE_TRANS : 0) | (exclude_self ? DN_EXCLUDE_SELF : 0);
  A.n_points = h->n_points;
  A.sums = d_sums.as<double>(); A.counts = d_counts.as<int>();
  {
    ProfScope ps("density");
    hipLaunchKernelGGL(density_k, dim3((unsigned)h->n_work), dim3(DN_QTILE), 0, st, A);
    IA3_KCHECK();
  }
  IA3_HIP(hipMemcpyAsync(sums, d_sums.p, 2 * n * sizeof(double), hipMemcpyDeviceToHost, st));
  IA3_HIP(hipMemcpyAsync(counts, d_counts.p, 2 * n * sizeof(int), hipMemcpyDeviceToHost, st));
  IA3_HIP(hipStreamSynchronize(st));
  return IA3_OK;
}

}  // extern "C"
