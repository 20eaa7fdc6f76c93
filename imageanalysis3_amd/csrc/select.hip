// Chromosome selection by candidate spots on the device: spot_tools/picking.py:767-794
// assign_spots_to_chromosomes and the loop of segmentation_tools/chromosome.py:377-399 select_candidate_chromosomes.
//   assign_k<PLAIN>     one lane per spot: owner = np.argmin(cdist(spot, candidates)) over all candidates
//   assign_k<FIRST>     the same, plus the round of the spot and cnt[round][owner] += 1; the add that finds 0 takes the round
//                       off lost[owner] (lost starts at R: the count is kept incrementally, never recomputed)
//   pick_k              one workgroup: the alive candidate with the largest lost (ties to the lowest index); it is removed
//                       when double(lost) / R > th, and the removal is recorded; otherwise the run is marked done
//   gather_k            the spots the removed candidate owned, compacted by wavefront ballot into a list
//   assign_k<REASSIGN>  one lane per listed spot: new owner among the alive candidates, cnt / lost updated as above
// The distance is SciPy's: sqrt((dz*dz + dx*dx) + dy*dy), every operation rounded to float64 on its own (this file is
// compiled without FMA contraction); a later candidate wins only when its ROOT is smaller, and the first NaN of a row
// wins it, as np.argmin has it.  Counts are int32 atomics: every result is the same on every run.
#include "ia3_rt.h"
#include "ia3_wave.h"
#include <chrono>
#include <math.h>
#include <vector>

using namespace ia3rt;

namespace {

constexpr int SEL_THREADS = 256;   // spots of a workgroup (IA3_SELECT_THREADS)
constexpr int SEL_TILE = 256;      // candidates staged in LDS at a time (IA3_SELECT_TILE)
constexpr int SEL_BATCH = 4;       // removal steps queued between two looks at the record
static_assert(SEL_THREADS == IA3_SELECT_THREADS && SEL_TILE == IA3_SELECT_TILE, "include/ia3.h states these sizes");

enum { PLAIN = 0, FIRST = 1, REASSIGN = 2 };

struct Ctl {
  unsigned long long visits;   // candidates visited (distance evaluations)
  int done;                    // 0 running, 1 nothing left above the threshold, 2 every candidate removed
  int removed;                 // candidate taken out by the last pick_k
  int n_removed, n_alive;
  unsigned m;                  // spots in the list of the last gather_k
};

struct Rec { int index, lost; };   // one removal; index -1: none

// np.argmin over one row of cdist, candidates visited in ascending index
struct Nearest {
  int c = -1;
  bool nan = false;
  double s = 0, r = 0;   // squared distance of c and its root
  __device__ inline void visit(int k, double dz, double dx, double dy) {
    const double q = (dz * dz + dx * dx) + dy * dy;
    if (nan) return;
    if (q != q) {            // the first NaN of the row
      c = k; nan = true;
    } else if (c < 0) {
      c = k; s = q; r = sqrt(q);
    } else if (q < s) {      // sqrt is monotone: only a smaller sum can have a smaller root, and not every one has
      const double t = sqrt(q);
      if (t < r) { c = k; s = q; r = t; }
    }
  }
};

// round of spot i: the r with round_start[r] <= i < round_start[r + 1] (empty rounds repeat a start)
__device__ inline int round_of(const int* __restrict__ round_start, int R, int i) {
  int lo = 0, hi = R;   // invariant: round_start[lo] <= i < round_start[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (round_start[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

// spots: n x 3 float64; cands: C x 3 float64.  PLAIN / FIRST: lane j takes spot j < n.  REASSIGN: lane j takes spot
// list[j], j < ctl->m, and only alive candidates are visited.  Every lane of a workgroup walks the same tiles.
template <int MODE>
__global__ __launch_bounds__(SEL_THREADS) void assign_k(const double* __restrict__ spots, int n, const double* __restrict__ cands,
                                                         int C, const int* __restrict__ alive, const int* __restrict__ round_start,
                                                         int R, const unsigned* __restrict__ list, int* __restrict__ owner,
                                                         int* __restrict__ rnd, int* __restrict__ cnt, int* __restrict__ lost,
                                                         Ctl* __restrict__ ctl) {
  __shared__ double s_z[SEL_TILE], s_x[SEL_TILE], s_y[SEL_TILE];
  __shared__ int s_alive[SEL_TILE];
  __shared__ unsigned s_visits;
  const int tid = threadIdx.x;
  unsigned total = (unsigned)n;
  if (MODE == REASSIGN) {
    if (ctl->done) return;
    total = ctl->m;
  }
  if (tid == 0) s_visits = 0;
  for (unsigned base = blockIdx.x * (unsigned)SEL_THREADS; base < total; base += gridDim.x * (unsigned)SEL_THREADS) {
    const unsigned j = base + (unsigned)tid;
    const bool live = j < total;
    int i = 0;
    double z = 0, x = 0, y = 0;
    if (live) {
      i = MODE == REASSIGN ? (int)list[j] : (int)j;
      const double* p = spots + (size_t)i * 3;
      z = p[0]; x = p[1]; y = p[2];
    }
    Nearest best;
    unsigned visits = 0;
    for (int c0 = 0; c0 < C; c0 += SEL_TILE) {
      const int w = C - c0 < SEL_TILE ? C - c0 : SEL_TILE;
      __syncthreads();
      for (int k = tid; k < w; k += SEL_THREADS) {
        const double* q = cands + (size_t)(c0 + k) * 3;
        s_z[k] = q[0]; s_x[k] = q[1]; s_y[k] = q[2];
        s_alive[k] = MODE == REASSIGN ? alive[c0 + k] : 1;
      }
      __syncthreads();
      if (live) {
        for (int k = 0; k < w; ++k) {
          if (MODE == REASSIGN && !s_alive[k]) continue;   // the same in every lane
          best.visit(c0 + k, z - s_z[k], x - s_x[k], y - s_y[k]);
          ++visits;
        }
      }
    }
    if (live) {
      owner[i] = best.c;
      if (MODE != PLAIN && best.c >= 0) {
        int r;
        if (MODE == FIRST) { r = round_of(round_start, R, i); rnd[i] = r; }
        else r = rnd[i];
        if (atomicAdd(cnt + (size_t)r * C + best.c, 1) == 0) atomicSub(lost + best.c, 1);
      }
    }
    if (MODE != PLAIN) {   // every live lane of a wavefront visited the same candidates: one add per wavefront
      const unsigned long long lanes = __ballot(live);
      if (lanes && (tid & 63) == __ffsll((long long)lanes) - 1)
        atomicAdd(&s_visits, visits * (unsigned)__popcll(lanes));   // at most 256 * C per pass: see the C limit below
      __syncthreads();
      if (tid == 0) {
        if (s_visits) atomicAdd(&ctl->visits, (unsigned long long)s_visits);
        s_visits = 0;
      }
    }
  }
}

__global__ void select_init_k(int* __restrict__ lost, int* __restrict__ alive, int C, int R, Ctl* __restrict__ ctl) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < C) { lost[c] = R; alive[c] = 1; }
  if (c == 0) {
    ctl->visits = 0; ctl->done = 0; ctl->removed = -1; ctl->n_removed = 0; ctl->n_alive = C; ctl->m = 0;
  }
}

// np.argmax of lost / R over the alive candidates (the largest lost, the lowest index among equals) and the test of
// chromosome.py:393 on it
__global__ __launch_bounds__(SEL_THREADS) void pick_k(const int* __restrict__ lost, int* __restrict__ alive, int C, int R, double th,
                                                       Rec* __restrict__ rec, Ctl* __restrict__ ctl) {
  __shared__ unsigned long long s_key[SEL_THREADS];
  if (ctl->done) return;
  const int tid = threadIdx.x;
  unsigned long long key = 0;   // 0: no alive candidate seen
  for (int c = tid; c < C; c += SEL_THREADS)
    if (alive[c]) {
      const unsigned long long k = ((unsigned long long)(unsigned)(lost[c] + 1) << 32) | (unsigned)(0x7fffffff - c);
      if (k > key) key = k;
    }
  s_key[tid] = key;
  __syncthreads();
  for (int h = SEL_THREADS / 2; h > 0; h >>= 1) {
    if (tid < h && s_key[tid + h] > s_key[tid]) s_key[tid] = s_key[tid + h];
    __syncthreads();
  }
  if (tid != 0) return;
  key = s_key[0];
  const int c = 0x7fffffff - (int)(unsigned)(key & 0xffffffffu);
  const int l = (int)(unsigned)(key >> 32) - 1;
  ctl->m = 0;
  if (key != 0 && (double)l / (double)R > th) {
    alive[c] = 0;
    rec[ctl->n_removed] = Rec{c, l};
    ctl->removed = c;
    ctl->n_removed += 1;
    ctl->n_alive -= 1;
    if (ctl->n_alive == 0) ctl->done = 2;
  } else {
    ctl->done = 1;
  }
}

__global__ __launch_bounds__(SEL_THREADS) void gather_k(const int* __restrict__ owner, int n, unsigned* __restrict__ list,
                                                         Ctl* __restrict__ ctl) {
  if (ctl->done) return;
  const int removed = ctl->removed;
  // n rounded up to whole wavefronts, so that a ballot always has 64 lanes behind it
  const unsigned span = ((unsigned)n + 63u) & ~63u;
  for (unsigned i = blockIdx.x * (unsigned)SEL_THREADS + threadIdx.x; i < span; i += gridDim.x * (unsigned)SEL_THREADS) {
    const bool hit = i < (unsigned)n && owner[i] == removed;
    const unsigned pos = ia3::wave_append(&ctl->m, hit);
    if (hit) list[pos] = i;
  }
}

inline unsigned spot_blocks(int n) {
  unsigned b = ((unsigned)n + SEL_THREADS - 1) / SEL_THREADS;
  const unsigned cap = (unsigned)num_cus() * 8u;
  if (cap >= 1 && b > cap) b = cap;
  return b < 1 ? 1 : b;
}

int check_tables(const double* spots, int n, const double* cands, int C) {
  if (n < 0 || C < 1) return set_error(IA3_EINVAL, "%d spots, %d candidates: at least one candidate is required", n, C);
  if ((n > 0 && !spots) || !cands) return set_error(IA3_EINVAL, "null table");
  if (C > (1 << 22)) return set_error(IA3_EUNSUPPORTED, "%d candidates: at most %d are built", C, 1 << 22);
  return IA3_OK;
}

double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

extern "C" {

int ia3_assign_nearest_dev(const double* spots_zxy, int n, const double* cands_zxy, int n_cand, int* owner) {
  int rc = ensure_init(); if (rc) return rc;
  rc = check_tables(spots_zxy, n, cands_zxy, n_cand); if (rc) return rc;
  if (n == 0) return IA3_OK;
  if (!owner) return set_error(IA3_EINVAL, "null owner table");
  hipStream_t st = stream();
  const size_t sb = (size_t)n * 3 * sizeof(double), cb = (size_t)n_cand * 3 * sizeof(double);
  Scratch d_spots(sb), d_cands(cb), d_owner((size_t)n * sizeof(int));
  if (!d_spots.p || !d_cands.p || !d_owner.p) return set_error(IA3_ENOMEM, "scratch for %d spots", n);
  IA3_HIP(hipMemcpyAsync(d_spots.p, spots_zxy, sb, hipMemcpyHostToDevice, st));
  IA3_HIP(hipMemcpyAsync(d_cands.p, cands_zxy, cb, hipMemcpyHostToDevice, st));
  {
    ProfScope ps("assign_nearest");
    hipLaunchKernelGGL((assign_k<PLAIN>), dim3(spot_blocks(n)), dim3(SEL_THREADS), 0, st, d_spots.as<double>(), n,
                       d_cands.as<double>(), n_cand, (const int*)nullptr, (const int*)nullptr, 0, (const unsigned*)nullptr,
                       d_owner.as<int>(), (int*)nullptr, (int*)nullptr, (int*)nullptr, (Ctl*)nullptr);
    IA3_KCHECK();
  }
  IA3_HIP(hipMemcpyAsync(owner, d_owner.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, st));
  IA3_HIP(hipStreamSynchronize(st));
  return IA3_OK;
}

int ia3_select_chromosomes_dev(const double* spots_zxy, const int* round_start, int n_rounds, const double* cands_zxy,
                               int n_cand, double loss_th, int* removed, int* removed_lost, int* n_removed, int* lost,
                               int* owner, long long* visits, double* times_ms) {
  int rc = ensure_init(); if (rc) return rc;
  if (n_rounds < 0 || !round_start || !removed || !removed_lost || !n_removed || !lost)
    return set_error(IA3_EINVAL, "select_chromosomes: null table or %d rounds", n_rounds);
  const int n = round_start[n_rounds];
  rc = check_tables(spots_zxy, n, cands_zxy, n_cand); if (rc) return rc;
  if (round_start[0] != 0) return set_error(IA3_EINVAL, "round_start[0] is %d, not 0", round_start[0]);
  for (int r = 0; r < n_rounds; ++r)
    if (round_start[r + 1] < round_start[r]) return set_error(IA3_EINVAL, "round_start falls at round %d", r);
  if ((long long)n_rounds * n_cand > 0x7fffffffLL)
    return set_error(IA3_EUNSUPPORTED, "%d rounds x %d candidates: the count table is limited to 2^31 - 1 entries", n_rounds, n_cand);
  const int C = n_cand, R = n_rounds;
  *n_removed = 0;
  if (visits) *visits = 0;
  if (times_ms) times_ms[0] = times_ms[1] = times_ms[2] = 0;
  if (R == 0) {   // np.mean of no rounds is NaN and nothing compares greater: every candidate stays
    for (int c = 0; c < C; ++c) lost[c] = 0;
    return IA3_OK;
  }
  hipStream_t st = stream();
  const size_t sb = (size_t)(n > 0 ? n : 1) * 3 * sizeof(double), cb = (size_t)C * 3 * sizeof(double);
  const size_t ib = (size_t)(n > 0 ? n : 1) * sizeof(int), nrec = (size_t)C + SEL_BATCH + 1;
  Scratch d_spots(sb), d_cands(cb), d_start((size_t)(R + 1) * sizeof(int)), d_owner(ib), d_rnd(ib), d_list(ib);
  Scratch d_cnt((size_t)R * C * sizeof(int)), d_lost((size_t)C * sizeof(int)), d_alive((size_t)C * sizeof(int));
  Scratch d_rec(nrec * sizeof(Rec)), d_ctl(sizeof(Ctl));
  if (!d_spots.p || !d_cands.p || !d_start.p || !d_owner.p || !d_rnd.p || !d_list.p || !d_cnt.p || !d_lost.p || !d_alive.p ||
      !d_rec.p || !d_ctl.p)
    return set_error(IA3_ENOMEM, "scratch for %d spots, %d rounds, %d candidates", n, R, C);
  Ctl* ctl = d_ctl.as<Ctl>();
  auto t0 = std::chrono::steady_clock::now();
  if (n > 0) IA3_HIP(hipMemcpyAsync(d_spots.p, spots_zxy, (size_t)n * 3 * sizeof(double), hipMemcpyHostToDevice, st));
  IA3_HIP(hipMemcpyAsync(d_cands.p, cands_zxy, cb, hipMemcpyHostToDevice, st));
  IA3_HIP(hipMemcpyAsync(d_start.p, round_start, (size_t)(R + 1) * sizeof(int), hipMemcpyHostToDevice, st));
  if (times_ms) {
    IA3_HIP(hipStreamSynchronize(st));
    times_ms[0] = ms_since(t0);
    t0 = std::chrono::steady_clock::now();
  }
  IA3_HIP(hipMemsetAsync(d_cnt.p, 0, (size_t)R * C * sizeof(int), st));
  IA3_HIP(hipMemsetAsync(d_rec.p, 0xff, nrec * sizeof(Rec), st));   // index -1 everywhere
  const unsigned blocks = spot_blocks(n);
  {
    ProfScope ps("select_first_pass");
    hipLaunchKernelGGL(select_init_k, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, st, d_lost.as<int>(), d_alive.as<int>(), C, R,
                       ctl);
    IA3_KCHECK();
    if (n > 0) {
      hipLaunchKernelGGL((assign_k<FIRST>), dim3(blocks), dim3(SEL_THREADS), 0, st, d_spots.as<double>(), n, d_cands.as<double>(),
                         C, (const int*)nullptr, d_start.as<int>(), R, (const unsigned*)nullptr, d_owner.as<int>(),
                         d_rnd.as<int>(), d_cnt.as<int>(), d_lost.as<int>(), ctl);
      IA3_KCHECK();
    }
  }
  if (times_ms) {
    IA3_HIP(hipStreamSynchronize(st));
    times_ms[1] = ms_since(t0);
    t0 = std::chrono::steady_clock::now();
  }
  // the removal loop: SEL_BATCH steps are queued (a step after the end does nothing), then their records are read
  std::vector<Rec> got(SEL_BATCH);
  int k = 0;
  bool done = false;
  while (!done) {
    {
      ProfScope ps("select_removal");
      for (int b = 0; b < SEL_BATCH; ++b) {
        hipLaunchKernelGGL(pick_k, dim3(1), dim3(SEL_THREADS), 0, st, d_lost.as<int>(), d_alive.as<int>(), C, R, loss_th,
                           d_rec.as<Rec>(), ctl);
        IA3_KCHECK();
        if (n > 0) {
          hipLaunchKernelGGL(gather_k, dim3(blocks), dim3(SEL_THREADS), 0, st, d_owner.as<int>(), n, d_list.as<unsigned>(), ctl);
          IA3_KCHECK();
          hipLaunchKernelGGL((assign_k<REASSIGN>), dim3(blocks), dim3(SEL_THREADS), 0, st, d_spots.as<double>(), n,
                             d_cands.as<double>(), C, d_alive.as<int>(), d_start.as<int>(), R, d_list.as<unsigned>(),
                             d_owner.as<int>(), d_rnd.as<int>(), d_cnt.as<int>(), d_lost.as<int>(), ctl);
          IA3_KCHECK();
        }
      }
    }
    IA3_HIP(hipMemcpyAsync(got.data(), d_rec.as<Rec>() + k, SEL_BATCH * sizeof(Rec), hipMemcpyDeviceToHost, st));
    IA3_HIP(hipStreamSynchronize(st));
    for (int b = 0; b < SEL_BATCH && !done; ++b) {
      if (got[b].index < 0) { done = true; break; }
      removed[k] = got[b].index;
      removed_lost[k] = got[b].lost;
      if (++k == C) done = true;
    }
  }
  *n_removed = k;
  if (times_ms) times_ms[2] = ms_since(t0);   // the last look has synchronised; the downloads below are not in it
  Ctl h;
  IA3_HIP(hipMemcpyAsync(&h, ctl, sizeof(Ctl), hipMemcpyDeviceToHost, st));
  IA3_HIP(hipMemcpyAsync(lost, d_lost.p, (size_t)C * sizeof(int), hipMemcpyDeviceToHost, st));
  if (owner && n > 0) IA3_HIP(hipMemcpyAsync(owner, d_owner.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, st));
  IA3_HIP(hipStreamSynchronize(st));
  if (visits) *visits = (long long)h.visits;
  if (h.n_removed != k) return set_error(IA3_EHIP, "select_chromosomes: %d removals recorded, %d read", h.n_removed, k);
  return k == C ? IA3_SELECT_EMPTY : IA3_OK;
}

}  // extern "C"
