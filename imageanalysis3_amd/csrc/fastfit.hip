// The fast path of External/Fitting_v4.py on resident stacks: box-normalised seeds (get_seed_points_base_v2, :100-126)
// and closed-form moment fits (gfit_fast :433-458, fast_fit_big_image :496-558).
//
// Seeds.  np.std of the stack from two fixed-order float64 reductions (FF_RED_BLOCKS blocks of 256 threads, every
// thread a fixed stride, LDS trees, then one block over the partial sums: the same operations in the same order on
// every run and every device, no floating-point atomics).  The test `v > std * th_seed, v > 0, v >= every neighbour
// within pix, neighbours taken modulo the shape` runs on LDS tiles whose halo is fetched through the wrapped index;
// survivors are appended by ballot + one integer atomic per wave and put in order on the host (they are few).
//
// Moment fits.  One wavefront per seed, up to BALL_SLOTS ball offsets per lane (ia3_ball.h).  The wave drops the offsets that
// belong to another seed's Voronoi cell (neighbour list, or a scan of the seed list for crowded seeds), gathers the
// voxels inside the image into LDS in ball order (ballot ranks), optionally re-centres on their first maximum, finds the
// order-statistic background by rank counting and leaves the sums to a few lanes that add serially in NumPy's order
// (ia3_fastfit.h, ia3_npsum.h): 254 additions per sum, where the order matters and the width does not.
#include "ia3_rt.h"
#include "ia3_fastfit.h"
#include "ia3_ball.h"
#include "ia3_wave.h"
#include <algorithm>
#include <math.h>

using namespace ia3rt;

namespace {

// ---- np.std ----------------------------------------------------------------------------------------------------
constexpr int FF_RED_BLOCKS = 256;

__device__ __forceinline__ double block_tree_256(double v, double* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] = sh[threadIdx.x] + sh[threadIdx.x + s];
    __syncthreads();
  }
  return sh[0];
}

// partial[b] = sum over the block's elements of x (mean == nullptr) or (x - *mean)^2
template <class T>
__global__ __launch_bounds__(256) void ff_partial_k(const T* __restrict__ im, size_t n, const double* __restrict__ mean,
                                                    double* __restrict__ partial) {
  __shared__ double sh[256];
  const double m = mean ? *mean : 0.0;
  double acc = 0.0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)FF_RED_BLOCKS * 256) {
    const double x = (double)im[i];
    if (mean) { const double d = x - m; acc = acc + d * d; }
    else acc = acc + x;
  }
  const double r = block_tree_256(acc, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = r;
}

// out[0] = (sum of the FF_RED_BLOCKS partial sums) / n
__global__ __launch_bounds__(256) void ff_final_k(const double* __restrict__ partial, double n, double* __restrict__ out) {
  __shared__ double sh[256];
  double acc = 0.0;
  for (int i = threadIdx.x; i < FF_RED_BLOCKS; i += 256) acc = acc + partial[i];
  const double r = block_tree_256(acc, sh);
  if (threadIdx.x == 0) out[0] = r / n;
}

// ---- local maxima with wrap-around neighbours -----------------------------------------------------------------
constexpr int SD_TZ = 4, SD_TX = 4, SD_TY = 64, SD_MAXPIX = 3;
constexpr int SD_LDS = (SD_TZ + 2 * SD_MAXPIX) * (SD_TX + 2 * SD_MAXPIX) * (SD_TY + 2 * SD_MAXPIX);

__device__ __forceinline__ int wrap(int i, int n) {   // Python's i % n
  int m = i % n;
  return m < 0 ? m + n : m;
}

struct SeedHit { long long idx; float h; int pad; };

template <class T>
__global__ __launch_bounds__(256) void ff_seed_k(const T* __restrict__ im, int Z, int X, int Y, int pix, double cutoff,
                                                 SeedHit* __restrict__ hits, unsigned cap, unsigned* __restrict__ count) {
  __shared__ float tile[SD_LDS];
  const int tz = SD_TZ + 2 * pix, tx = SD_TX + 2 * pix, ty = SD_TY + 2 * pix;
  const int z0 = blockIdx.z * SD_TZ, x0 = blockIdx.y * SD_TX, y0 = blockIdx.x * SD_TY;
  for (int e = threadIdx.x; e < tz * tx * ty; e += 256) {
    const int c = e % ty, r = (e / ty) % tx, p = e / (ty * tx);
    tile[e] = (float)im[((size_t)wrap(z0 - pix + p, Z) * X + wrap(x0 - pix + r, X)) * Y + wrap(y0 - pix + c, Y)];
  }
  __syncthreads();
  const int ly = threadIdx.x & 63, lx = threadIdx.x >> 6;
  for (int lz = 0; lz < SD_TZ; ++lz) {
    const int z = z0 + lz, x = x0 + lx, y = y0 + ly;
    bool keep = z < Z && x < X && y < Y;
    float v = 0.0f;
    if (keep) {
      v = tile[((lz + pix) * tx + lx + pix) * ty + ly + pix];
      keep = (double)v > cutoff && v > 0.0f;
      for (int dz = 0; dz <= 2 * pix && keep; ++dz)
        for (int dx = 0; dx <= 2 * pix && keep; ++dx) {
          const float* row = tile + ((lz + dz) * tx + lx + dx) * ty + ly;
          for (int dy = 0; dy <= 2 * pix; ++dy) keep = keep && v >= row[dy];
        }
    }
    const unsigned pos = ia3::wave_append(count, keep);
    if (keep && pos < cap) hits[pos] = SeedHit{((long long)z * X + x) * Y + y, v, 0};
  }
}

// ---- neighbour lists: one wave per seed scans all seeds 64 at a time; ballot + prefix rank, so every list is in
// ascending index order (what query_ball_tree returns, self left out here) ---------------------------------------
__global__ __launch_bounds__(256) void ff_nbr_k(const double* __restrict__ seeds, int n, double r2, int* __restrict__ cnt,
                                                int* __restrict__ idx) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;   // whole wave leaves together
  int c = 0;
  ia3::scan_seeds(seeds, 0, n, i, r2, [&](int j0, unsigned long long m, bool hit) {
    if (hit) {
      const int pos = c + ia3::lane_rank(m);
      if (pos < ia3::BALL_NBLIST) idx[(size_t)i * ia3::BALL_NBLIST + pos] = j0 + lane;
    }
    c += __popcll(m);
    return true;
  });
  if (lane == 0) cnt[i] = c;   // not clamped: > BALL_NBLIST = the list overflowed, the consumer scans
}

// ---- moment fit ----------------------------------------------------------------------------------------------------
struct FfLds {
  double v[ia3::FF_MAXVOX];      // voxel values, list order
  double wn[ia3::FF_MAXVOX];     // normalised weights
  int x[3][ia3::FF_MAXVOX];      // voxel coordinates
  double bk, h, c[3];
};

// the 12 numbers of gfit_fast from the n voxels in LDS (n <= FF_MAXVOX); called by every lane of the wave
__device__ __forceinline__ void moments_from_lds(FfLds* L, int n, double bk_f, int kind, double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  if (n == 0) {
    if (lane < 12) out[lane] = __builtin_nan("");
    return;
  }
  const int k = (int)((double)n * bk_f);
  for (int e = lane; e < n; e += 64)
    if (ia3::ff_is_kth(L->v, n, e, k)) L->bk = L->v[e];   // equal values only: any writer leaves the same bits
  __syncthreads();
  if (lane == 0) L->h = ia3::ff_weights(L->v, n, L->bk, kind, L->wn);
  __syncthreads();
  if (lane < 3) L->c[lane] = ia3::ff_centroid(L->x[lane], L->wn, n);
  __syncthreads();
  if (lane < 6) {
    // a, b, c, d, e, f = Cov[0][0], [1][1], [2][2], [0][1], [0][2], [1][2]
    const int i = lane < 3 ? lane : (lane == 5 ? 1 : 0), j = lane < 3 ? lane : (lane == 3 ? 1 : 2);
    out[5 + lane] = ia3::ff_cov(L->x[i], L->c[i], L->x[j], L->c[j], L->wn, n);
  } else if (lane == 6) {
    out[0] = L->h; out[1] = L->c[0]; out[2] = L->c[1]; out[3] = L->c[2]; out[4] = L->bk; out[11] = __builtin_nan("");
  }
}

struct MomentArgs {
  const void* im; int Z, X, Y;
  const double* centers; int n;
  const int* ball; int nball;
  int avoid, recenter, kind;
  double bk_f;
  const int* nbr_cnt; const int* nbr_idx; int nb_cap; double nb_r2;
  double* out12;
  int* vox_count; double* vox_vals; int* vox_zxy;   // optional: the voxel list each seed was fitted on (nball slots per seed)
};

template <class T>
__global__ __launch_bounds__(64) void ff_moment_k(MomentArgs a) {
  __shared__ FfLds L;
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x;
  if (i >= a.n) return;
  const T* __restrict__ im = (const T*)a.im;
  const double c0 = a.centers[3 * i], c1 = a.centers[3 * i + 1], c2 = a.centers[3 * i + 2];
  int iz = (int)c0, ix = (int)c1, iy = (int)c2;   // Python int(): toward zero

  // ball offsets of this lane that stay with this seed (bit s = slot s)
  ia3::SeedBall sb{a.ball, a.nball, iz, ix, iy, a.Z, a.X, a.Y};
  unsigned own = 0;
  for (int s = 0; s < ia3::BALL_SLOTS; ++s)
    if (sb.has(s)) own |= 1u << s;
  if (a.avoid)
    ia3::each_neighbour(a.centers, i, a.nbr_cnt, a.nbr_idx, a.nb_cap, a.nb_r2, [&]() { return ia3::SeedRange{0, a.n}; }, [&](int j) {
      // wave-uniform j != i: argmin over the ascending neighbour list takes the first minimum
      const double dz = a.centers[3 * j] - c0, dx = a.centers[3 * j + 1] - c1, dy = a.centers[3 * j + 2] - c2;
      for (int s = 0; s < ia3::BALL_SLOTS; ++s)
        if (sb.has(s)) {
          const ia3::BallOff o = sb.off(s);
          if (ia3::ff_loses(dz, dx, dy, o.dz, o.dx, o.dy, j < i)) own &= ~(1u << s);
        }
      return true;
    });

  int n = 0;
  for (int pass = 0; pass < 2; ++pass) {
    n = 0;
    sb.iz = iz; sb.ix = ix; sb.iy = iy;   // pass 1: re-centred
    for (int s = 0; s < ia3::BALL_SLOTS; ++s) {
      bool in = false;
      int z = 0, x = 0, y = 0;
      if ((own >> s) & 1u) sb.voxel(s, [&](int vz, int vx, int vy, bool inside) { z = vz; x = vx; y = vy; in = inside; });
      const unsigned long long m = __ballot(in);
      if (in) {
        const int pos = n + ia3::lane_rank(m);   // < nball <= FF_MAXVOX
        L.v[pos] = (double)im[((size_t)z * a.X + x) * a.Y + y];
        L.x[0][pos] = z; L.x[1][pos] = x; L.x[2][pos] = y;
      }
      n += __popcll(m);
    }
    __syncthreads();
    if (pass == 1 || !a.recenter || n == 0) break;
    // np.argmax: the first maximum of the list
    double bv = 0.0;
    int be = 0x7fffffff;
    for (int e = lane; e < n; e += 64)
      if (be == 0x7fffffff || L.v[e] > bv) { bv = L.v[e]; be = e; }
    for (int d = 32; d > 0; d >>= 1) {
      const double ov = __shfl_xor(bv, d);
      const int oe = __shfl_xor(be, d);
      if (oe != 0x7fffffff && (be == 0x7fffffff || ov > bv || (ov == bv && oe < be))) { bv = ov; be = oe; }
    }
    iz = L.x[0][be]; ix = L.x[1][be]; iy = L.x[2][be];
    __syncthreads();
  }

  if (a.vox_count) {
    if (lane == 0) a.vox_count[i] = n;
    for (int e = lane; e < n; e += 64) {
      const size_t o = (size_t)i * a.nball + e;
      a.vox_vals[o] = L.v[e];
      a.vox_zxy[3 * o] = L.x[0][e]; a.vox_zxy[3 * o + 1] = L.x[1][e]; a.vox_zxy[3 * o + 2] = L.x[2][e];
    }
  }
  moments_from_lds(&L, n, a.bk_f, a.kind, a.out12 + 12 * (size_t)i);
}

// gfit_fast on one explicit voxel list (n <= FF_MAXVOX)
__global__ __launch_bounds__(64) void ff_voxels_k(const double* __restrict__ vals, const int* __restrict__ coords, int n,
                                                  int kind, double bk_f, double* __restrict__ out12) {
  __shared__ FfLds L;
  for (int e = threadIdx.x; e < n; e += 64) {
    L.v[e] = vals[e];
    L.x[0][e] = coords[3 * e]; L.x[1][e] = coords[3 * e + 1]; L.x[2][e] = coords[3 * e + 2];
  }
  __syncthreads();
  moments_from_lds(&L, n, bk_f, kind, out12);
}

template <class T>
int stack_std(const T* d, size_t n, double* d_tmp, double* var_out, hipStream_t st) {
  // d_tmp: FF_RED_BLOCKS partial sums, then [mean, variance]
  double* stats = d_tmp + FF_RED_BLOCKS;
  hipLaunchKernelGGL((ff_partial_k<T>), dim3(FF_RED_BLOCKS), dim3(256), 0, st, d, n, (const double*)nullptr, d_tmp);
  hipLaunchKernelGGL(ff_final_k, dim3(1), dim3(256), 0, st, (const double*)d_tmp, (double)n, stats);
  hipLaunchKernelGGL((ff_partial_k<T>), dim3(FF_RED_BLOCKS), dim3(256), 0, st, d, n, (const double*)stats, d_tmp);
  hipLaunchKernelGGL(ff_final_k, dim3(1), dim3(256), 0, st, (const double*)d_tmp, (double)n, stats + 1);
  IA3_KCHECK();
  IA3_HIP(hipMemcpyAsync(var_out, stats + 1, sizeof(double), hipMemcpyDeviceToHost, st));
  IA3_HIP(hipStreamSynchronize(st));
  return IA3_OK;
}

}  // namespace

extern "C" {

int ia3_fastfit_normalize_dev(const ia3_stack* im, int sz, ia3_stack** out) {
  int rc = ensure_init(); if (rc) return rc;
  if (!im || !out) return set_error(IA3_EINVAL, "null argument");
  if (sz < 1 || sz > IA3_BLUR_MAX_GB)
    return set_error(IA3_EUNSUPPORTED, "normalzie_im: box size %d outside the supported range 1..%d", sz, IA3_BLUR_MAX_GB);
  ia3_stack* o = nullptr;
  rc = ia3_stack_alloc(IA3_F32, im->Z, im->X, im->Y, &o); if (rc) return rc;
  rc = ia3k::blurnorm_planes(im->d, im->dtype, im->Z, im->X, im->Y, sz, IA3_BLUR_SUBTRACT, (float*)o->d);
  if (rc) { ia3_stack_free(o); return rc; }
  *out = o;
  return IA3_OK;
}

int ia3_fastfit_seeds_dev(const ia3_stack* im, int gfilt_size, int filt_size, double th_seed, int th_f32, int max_num,
                          double* zxyh, int capacity, int* n_out, double* std_out) {
  int rc = ensure_init(); if (rc) return rc;
  if (!im || !n_out || !std_out || (capacity > 0 && !zxyh) || capacity < 0) return set_error(IA3_EINVAL, "bad argument");
  if (gfilt_size < 0 || gfilt_size > IA3_BLUR_MAX_GB)
    return set_error(IA3_EUNSUPPORTED, "get_seed_points_base_v2: gfilt_size %d outside the supported range 0..%d", gfilt_size, IA3_BLUR_MAX_GB);
  if (filt_size < 0) return set_error(IA3_EINVAL, "filt_size must be >= 0");
  const int pix = filt_size / 2;
  if (pix > SD_MAXPIX)
    return set_error(IA3_EUNSUPPORTED, "get_seed_points_base_v2: filt_size %d (neighbours within %d) above the supported %d", filt_size, pix, 2 * SD_MAXPIX + 1);
  const int Z = im->Z, X = im->X, Y = im->Y;
  const size_t nvox = (size_t)Z * X * Y;
  if (nvox == 0) return set_error(IA3_EINVAL, "empty stack");
  hipStream_t st = stream();
  const void* src = im->d;
  int dtype = im->dtype;
  Scratch norm(gfilt_size ? nvox * sizeof(float) : 16);
  if (!norm.p) return IA3_ENOMEM;
  if (gfilt_size) {
    rc = ia3k::blurnorm_planes(im->d, im->dtype, Z, X, Y, gfilt_size, IA3_BLUR_SUBTRACT, norm.as<float>()); if (rc) return rc;
    src = norm.p;
    dtype = IA3_F32;
  }
  Scratch red((FF_RED_BLOCKS + 2) * sizeof(double));
  if (!red.p) return IA3_ENOMEM;
  double var = 0.0;
  {
    ProfScope ps("fastfit_std");
    rc = dtype == IA3_U16 ? stack_std((const uint16_t*)src, nvox, red.as<double>(), &var, st)
                          : stack_std((const float*)src, nvox, red.as<double>(), &var, st);
    if (rc) return rc;
  }
  // np.std returns float32 for a float32 stack, float64 for uint16; std_ * th_seed stays float32 for a Python number
  double sd = sqrt(var), cutoff;
  if (dtype == IA3_F32) {
    const float sf = (float)sd;
    sd = (double)sf;
    cutoff = th_f32 ? (double)(sf * (float)th_seed) : sd * th_seed;
  } else {
    cutoff = sd * th_seed;
  }
  *std_out = sd;

  const size_t cap = std::min(nvox, (size_t)1 << 22);
  Scratch hits(cap * sizeof(SeedHit) + sizeof(unsigned));
  if (!hits.p) return IA3_ENOMEM;
  unsigned* d_count = (unsigned*)((char*)hits.p + cap * sizeof(SeedHit));
  IA3_HIP(hipMemsetAsync(d_count, 0, sizeof(unsigned), st));
  {
    ProfScope ps("fastfit_seed");
    const dim3 g((Y + SD_TY - 1) / SD_TY, (X + SD_TX - 1) / SD_TX, (Z + SD_TZ - 1) / SD_TZ);
    if (g.y > 65535u || g.z > 65535u) return set_error(IA3_EUNSUPPORTED, "stack too large for the seed grid");
    if (dtype == IA3_U16)
      hipLaunchKernelGGL((ff_seed_k<uint16_t>), g, dim3(256), 0, st, (const uint16_t*)src, Z, X, Y, pix, cutoff, hits.as<SeedHit>(), (unsigned)cap, d_count);
    else
      hipLaunchKernelGGL((ff_seed_k<float>), g, dim3(256), 0, st, (const float*)src, Z, X, Y, pix, cutoff, hits.as<SeedHit>(), (unsigned)cap, d_count);
    IA3_KCHECK();
  }
  unsigned cnt = 0;
  IA3_HIP(hipMemcpyAsync(&cnt, d_count, sizeof(unsigned), hipMemcpyDeviceToHost, st));
  IA3_HIP(hipStreamSynchronize(st));
  if (cnt > cap) return set_error(IA3_ECAPACITY, "%u local maxima above the cutoff (more than %zu): raise th_seed", cnt, cap);
  std::vector<SeedHit> h(cnt);
  if (cnt) {
    IA3_HIP(hipMemcpyAsync(h.data(), hits.p, cnt * sizeof(SeedHit), hipMemcpyDeviceToHost, st));
    IA3_HIP(hipStreamSynchronize(st));
  }
  // brightest first; equal heights in descending voxel order (a stable ascending argsort, reversed)
  std::sort(h.begin(), h.end(), [](const SeedHit& a, const SeedHit& b) { return a.h != b.h ? a.h > b.h : a.idx > b.idx; });
  size_t keep = h.size();
  if (max_num >= 0 && (size_t)max_num < keep) keep = (size_t)max_num;
  *n_out = (int)keep;
  if (keep > (size_t)capacity) return set_error(IA3_ECAPACITY, "%zu seeds, room for %d", keep, capacity);
  for (size_t k = 0; k < keep; ++k) {
    const long long idx = h[k].idx;
    zxyh[4 * k] = (double)(idx / ((long long)X * Y));
    zxyh[4 * k + 1] = (double)((idx / Y) % X);
    zxyh[4 * k + 2] = (double)(idx % Y);
    zxyh[4 * k + 3] = (double)h[k].h;
  }
  return IA3_OK;
}

int ia3_fastfit_moments_dev(const ia3_stack* im, const double* centers_zxy, int n, int radius_fit, int avoid_neighbors,
                            int recenter, double bk_f, double* out12, int* vox_count, double* vox_vals, int* vox_zxy) {
  int rc = ensure_init(); if (rc) return rc;
  if (!im || n < 0 || (n > 0 && (!centers_zxy || !out12))) return set_error(IA3_EINVAL, "bad argument");
  if (vox_count && (!vox_vals || !vox_zxy)) return set_error(IA3_EINVAL, "vox_count needs vox_vals and vox_zxy");
  if (radius_fit < 1) return set_error(IA3_EINVAL, "radius_fit must be >= 1");
  if (!(bk_f >= 0.0 && bk_f < 1.0)) return set_error(IA3_EINVAL, "bk_f must lie in [0, 1)");
  std::vector<int> ball;
  const int nball = radius_fit <= 5 ? ia3::ball_build(radius_fit, ball) : ia3::FF_MAXVOX + 1;
  if (nball > ia3::FF_MAXVOX)
    return set_error(IA3_EUNSUPPORTED, "fast_fit_big_image: radius_fit %d gives more than %d voxels per ball", radius_fit, ia3::FF_MAXVOX);
  if (n == 0) return IA3_OK;
  if (n > 0x7fffffff / ia3::BALL_NBLIST) return set_error(IA3_EUNSUPPORTED, "too many seeds");   // each_neighbour indexes with int
  for (int k = 0; k < 3 * n; ++k)
    if (!(fabs(centers_zxy[k]) < 1e9)) return set_error(IA3_EINVAL, "centre %d is not a finite voxel position", k / 3);
  hipStream_t st = stream();
  const size_t nn = (size_t)n;
  Scratch dcen(nn * 3 * sizeof(double)), dball((size_t)nball * sizeof(int)), dout(nn * 12 * sizeof(double)),
      dcnt(nn * sizeof(int)), didx(avoid_neighbors ? nn * ia3::BALL_NBLIST * sizeof(int) : 16),
      dvc(vox_count ? nn * sizeof(int) : 16), dvv(vox_count ? nn * nball * sizeof(double) : 16),
      dvx(vox_count ? nn * nball * 3 * sizeof(int) : 16);
  if (!dcen.p || !dball.p || !dout.p || !dcnt.p || !didx.p || !dvc.p || !dvv.p || !dvx.p) return IA3_ENOMEM;
  IA3_HIP(hipMemcpyAsync(dcen.p, centers_zxy, nn * 3 * sizeof(double), hipMemcpyHostToDevice, st));
  IA3_HIP(hipMemcpyAsync(dball.p, ball.data(), (size_t)nball * sizeof(int), hipMemcpyHostToDevice, st));
  const double rr = 2.0 * (double)radius_fit;
  if (avoid_neighbors) {
    ProfScope ps("fastfit_nbr");
    hipLaunchKernelGGL(ff_nbr_k, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, dcen.as<double>(), n, rr * rr, dcnt.as<int>(), didx.as<int>());
    IA3_KCHECK();
  }
  MomentArgs a;
  a.im = im->d; a.Z = im->Z; a.X = im->X; a.Y = im->Y;
  a.centers = dcen.as<double>(); a.n = n;
  a.ball = dball.as<int>(); a.nball = nball;
  a.avoid = avoid_neighbors ? 1 : 0; a.recenter = recenter ? 1 : 0; a.kind = im->dtype == IA3_U16 ? 1 : 0;
  a.bk_f = bk_f;
  a.nbr_cnt = dcnt.as<int>(); a.nbr_idx = didx.as<int>(); a.nb_cap = ia3k::get_fit_nblist(); a.nb_r2 = rr * rr;
  a.out12 = dout.as<double>();
  a.vox_count = vox_count ? dvc.as<int>() : nullptr; a.vox_vals = dvv.as<double>(); a.vox_zxy = dvx.as<int>();
  {
    ProfScope ps("fastfit_moment");
    if (im->dtype == IA3_U16) hipLaunchKernelGGL((ff_moment_k<uint16_t>), dim3((unsigned)n), dim3(64), 0, st, a);
    else hipLaunchKernelGGL((ff_moment_k<float>), dim3((unsigned)n), dim3(64), 0, st, a);
    IA3_KCHECK();
  }
  IA3_HIP(hipMemcpyAsync(out12, dout.p, nn * 12 * sizeof(double), hipMemcpyDeviceToHost, st));
  if (vox_count) {
    IA3_HIP(hipMemcpyAsync(vox_count, dvc.p, nn * sizeof(int), hipMemcpyDeviceToHost, st));
    IA3_HIP(hipMemcpyAsync(vox_vals, dvv.p, nn * nball * sizeof(double), hipMemcpyDeviceToHost, st));
    IA3_HIP(hipMemcpyAsync(vox_zxy, dvx.p, nn * nball * 3 * sizeof(int), hipMemcpyDeviceToHost, st));
  }
  IA3_HIP(hipStreamSynchronize(st));
  return IA3_OK;
}

int ia3_fastfit_voxels(const double* vals, const int* coords_zxy, int n, int kind, double bk_f, double* out12) {
  int rc = ensure_init(); if (rc) return rc;
  if (n < 0 || !out12 || (n > 0 && (!vals || !coords_zxy))) return set_error(IA3_EINVAL, "bad argument");
  if (kind < 0 || kind > 2) return set_error(IA3_EINVAL, "kind %d: 0 float32, 1 uint16, 2 float64", kind);
  if (!(bk_f >= 0.0 && bk_f < 1.0)) return set_error(IA3_EINVAL, "bk_f must lie in [0, 1)");
  if (n > ia3::FF_MAXVOX) return set_error(IA3_EUNSUPPORTED, "gfit_fast: %d voxels (> %d)", n, ia3::FF_MAXVOX);
  hipStream_t st = stream();
  const size_t m = (size_t)(n ? n : 1);
  Scratch dv(m * sizeof(double)), dc(m * 3 * sizeof(int)), dout(12 * sizeof(double));
  if (!dv.p || !dc.p || !dout.p) return IA3_ENOMEM;
  if (n) {
    IA3_HIP(hipMemcpyAsync(dv.p, vals, (size_t)n * sizeof(double), hipMemcpyHostToDevice, st));
    IA3_HIP(hipMemcpyAsync(dc.p, coords_zxy, (size_t)n * 3 * sizeof(int), hipMemcpyHostToDevice, st));
  }
  {
    ProfScope ps("fastfit_voxels");
    hipLaunchKernelGGL(ff_voxels_k, dim3(1), dim3(64), 0, st, (const double*)dv.as<double>(), (const int*)dc.as<int>(), n, kind, bk_f, dout.as<double>());
    IA3_KCHECK();
  }
  IA3_HIP(hipMemcpyAsync(out12, dout.p, 12 * sizeof(double), hipMemcpyDeviceToHost, st));
  IA3_HIP(hipStreamSynchronize(st));
  return IA3_OK;
}

}  // extern "C"
