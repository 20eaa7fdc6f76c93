// The seed ball: the integer ball around a truncated seed position that every fit walks (External/Fitting_v4.py:506-508,
// :590-600), its voxel-to-(lane, slot) map, its tests against the image and against other seeds, and the neighbour
// iteration of the wave that owns it.  The one statement of each; fit.hip and fastfit.hip call these, except in
// fit_stages_k's gather_first and gather_repeat (fit.hip), which keep the walk written out and say why.
// Map: one wavefront holds one ball; ball voxel vi (reference order) sits in slot vi / 64 of lane vi % 64.  A per-lane
// bit set over slots (`valid`, `lost`, `own`: bit s = slot s) and a per-slot lane mask (a ballot; fit.hip's tie_lost:
// word = slot, bit = lane) name the same voxels; ball_vi / ball_slot / ball_lane are the map, nothing else restates it.
// Host/device agnostic (tests/native/fastfit_cpu.cpp builds it with g++) down to `#ifdef __HIPCC__`, wave code from there.
#pragma once
#include <vector>
#include "ia3_fastfit.h"

namespace ia3 {

constexpr int BALL_LANES = 64, BALL_SLOTS = 8;          // voxel slots per lane
constexpr int BALL_MAXVOX = BALL_LANES * BALL_SLOTS;    // radius 5: 512 voxels
constexpr int BALL_NBLIST = 64;   // neighbour slots per seed (seeds within 2r); denser seeds re-scan the seed list instead
static_assert(FF_MAXVOX == BALL_MAXVOX, "the moment fit's voxel list holds one ball");

IA3_HD int ball_vi(int lane, int s) { return lane + 64 * s; }
IA3_HD int ball_slot(int vi) { return vi / 64; }
IA3_HD int ball_lane(int vi) { return vi % 64; }

// offsets of a ball voxel from the truncated seed position, one word per voxel: signed bytes dz, dx, dy, 0
struct BallOff { int dz, dx, dy; };
IA3_HD int ball_pack(int dz, int dx, int dy) { return (dz & 0xff) | ((dx & 0xff) << 8) | ((dy & 0xff) << 16); }
IA3_HD BallOff ball_off(const int* ball, int vi) {
  const int w = ball[vi];
  return BallOff{(int)(signed char)(w & 0xff), (int)(signed char)((w >> 8) & 0xff), (int)(signed char)((w >> 16) & 0xff)};
}

// the reference's ball in its order: [-r, r) per axis in np.indices order, d^2 <= r^2.  Returns the number of voxels.
inline int ball_build(int r, std::vector<int>& ball) {
  ball.clear();
  for (int z = -r; z < r; ++z)
    for (int x = -r; x < r; ++x)
      for (int y = -r; y < r; ++y)
        if (z * z + x * x + y * y <= r * r) ball.push_back(ball_pack(z, x, y));
  return (int)ball.size();
}

// is the offset (oz, ox, oy) from a truncated seed position a voxel of that seed's ball?
IA3_HD bool in_ball(int oz, int ox, int oy, int r) {
  return oz >= -r && oz < r && ox >= -r && ox < r && oy >= -r && oy < r && oz * oz + ox * ox + oy * oy <= r * r;
}

// The ball of the seed truncated to (iz, ix, iy) in a Z x X x Y image.  at / voxel hand f(z, x, y, inside) the position
// of ball voxel vi / of this lane's slot s and whether it lies in the image; nothing is handed over for vi >= nball (the
// rest of a partly filled slot and the slots behind it).
struct SeedBall {
  const int* ball; int nball, iz, ix, iy, Z, X, Y;
  template <class F>
  IA3_HD void at(int vi, F f) const {
    if (vi < nball) {
      const BallOff o = ball_off(ball, vi);
      const int z = iz + o.dz, x = ix + o.dx, y = iy + o.dy;
      f(z, x, y, z >= 0 && z < Z && x >= 0 && x < X && y >= 0 && y < Y);
    }
  }
#ifdef __HIPCC__
  template <class F>
  __device__ __forceinline__ void voxel(int s, F f) const { at(ball_vi(threadIdx.x & 63, s), f); }
  __device__ __forceinline__ bool has(int s) const { return ball_vi(threadIdx.x & 63, s) < nball; }   // slot s is in the table
  __device__ __forceinline__ BallOff off(int s) const { return ball_off(ball, ball_vi(threadIdx.x & 63, s)); }   // where has(s)
#endif
};

#ifdef __HIPCC__
// number of voxels of the wave's ball from every lane's slot bits
__device__ __forceinline__ int ball_count(unsigned valid) {
  return __popcll(__ballot(valid & 1u)) + __popcll(__ballot(valid & 2u)) + __popcll(__ballot(valid & 4u)) +
         __popcll(__ballot(valid & 8u)) + __popcll(__ballot(valid & 16u)) + __popcll(__ballot(valid & 32u)) +
         __popcll(__ballot(valid & 64u)) + __popcll(__ballot(valid & 128u));
}

// Squared distance as scipy's cKDTree forms it (query.cxx: s = 0; s += d_k * d_k for k = 0, 1, 2; separate multiply and
// add): the Voronoi decisions compare these values for equality, so no contraction into fused multiply-adds here.
__device__ __forceinline__ double dist2_seq(double az, double ax, double ay, double bz, double bx, double by) {
  const double d0 = az - bz, d1 = ax - bx, d2 = ay - by;
  return __dadd_rn(__dadd_rn(__dmul_rn(d0, d0), __dmul_rn(d1, d1)), __dmul_rn(d2, d2));
}

// Voronoi (Fitting_v4.py:612, :422-424): the lane's slots whose voxel is strictly nearer to the seed at s than to the
// ball's own seed at c (`lost`), or exactly as near (`tied`).  Every voxel of the table counts, inside the image or not.
struct BallSplit { unsigned lost, tied; };
__device__ __forceinline__ BallSplit ball_voronoi(const SeedBall& sb, const double* c, const double* s) {
  BallSplit r{0u, 0u};
#pragma unroll
  for (int k = 0; k < BALL_SLOTS; ++k)
    sb.voxel(k, [&](int vz, int vx, int vy, bool) {
      const double z = (double)vz, x = (double)vx, y = (double)vy;
      const double dme = dist2_seq(c[0], c[1], c[2], z, x, y);
      const double dj = dist2_seq(s[0], s[1], s[2], z, x, y);
      if (dj < dme) r.lost |= 1u << k;
      else if (dj == dme) r.tied |= 1u << k;
    });
  return r;
}
__device__ __forceinline__ bool voronoi_tied(const double* c, const double* s, int z, int x, int y) {   // the tie half alone
  return dist2_seq(c[0], c[1], c[2], (double)z, (double)x, (double)y) == dist2_seq(s[0], s[1], s[2], (double)z, (double)x, (double)y);
}

// f(j) for every set bit b of a ballot over the seeds j0 + lane, ascending, wave-uniform; false from f stops and is returned
template <class F>
__device__ __forceinline__ bool each_hit(int j0, unsigned long long m, F f) {
  while (m) {
    const int b = __ffsll((long long)m) - 1;
    m &= m - 1;
    if (!f(j0 + b)) return false;
  }
  return true;
}

// One wave scans the seeds [first, last) 64 at a time for those within sqrt(r2) of seed i (itself left out) and hands
// f(j0, ballot, hit) every step: bit b = seed j0 + b is a neighbour, hit = the lane's own bit.  false from f stops the scan.
template <class F>
__device__ __forceinline__ void scan_seeds(const double* seeds, int first, int last, int i, double r2, F f) {
  const int lane = threadIdx.x & 63;
  const double cz = seeds[3 * i], cx = seeds[3 * i + 1], cy = seeds[3 * i + 2];
  for (int j0 = first; j0 < last; j0 += 64) {
    const int j = j0 + lane;
    bool hit = false;
    if (j < last && j != i) {
      const double a = cz - seeds[3 * j], b = cx - seeds[3 * j + 1], d = cy - seeds[3 * j + 2];
      hit = a * a + b * b + d * d <= r2;
    }
    if (!f(j0, __ballot(hit), hit)) return;
  }
}

// f(j) for every seed j != i within 2r of seed i, ascending j, wave-uniform.  Seeds with at most nb_cap (<= BALL_NBLIST)
// neighbours read their list; denser ones (the reference has no cap: it queries a cKDTree) scan the seed range that
// range() names — asked only then — 64 candidates per step.  f returns false to stop early.
struct SeedRange { int first, last; };
template <class R, class F>
__device__ __forceinline__ void each_neighbour(const double* seeds, int i, const int* nbr_cnt, const int* nbr_idx, int nb_cap, double r2, R range, F f) {
  const int cnt = nbr_cnt[i];
  if (cnt <= nb_cap) {
    for (int q = i * BALL_NBLIST; q < i * BALL_NBLIST + cnt; ++q)   // (int: this form keeps fit_stages_k's instructions)
      if (!f(nbr_idx[q])) return;
    return;
  }
  const SeedRange sr = range();
  scan_seeds(seeds, sr.first, sr.last, i, r2, [&](int j0, unsigned long long m, bool) { return each_hit(j0, m, f); });
}
#endif  // __HIPCC__

}  // namespace ia3
