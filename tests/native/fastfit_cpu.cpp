// TEST INFRASTRUCTURE — host build of the moment fit's arithmetic (csrc/ia3_fastfit.h), of NumPy's summation order
// (csrc/ia3_npsum.h) and of the seed ball's table and voxel-to-lane map (csrc/ia3_ball.h), the headers fastfit.hip and
// fit.hip compile for the device, so they can be compared with NumPy and with the reference's rows on the CPU.  Not
// shipped, not a fallback.
#include <vector>
#include "../../imageanalysis3_amd/csrc/ia3_fastfit.h"
#include "../../imageanalysis3_amd/csrc/ia3_ball.h"

// the seed ball of radius r: its packed words (at most cap are written); returns the number of voxels
extern "C" int ia3cpu_ball_table(int r, int* words, int cap) {
  std::vector<int> ball;
  const int n = ia3::ball_build(r, ball);
  for (int k = 0; k < n && k < cap; ++k) words[k] = ball[(size_t)k];
  return n;
}
extern "C" void ia3cpu_ball_off(const int* words, int vi, int* dzxy) {
  const ia3::BallOff o = ia3::ball_off(words, vi);
  dzxy[0] = o.dz; dzxy[1] = o.dx; dzxy[2] = o.dy;
}
extern "C" int ia3cpu_ball_slot(int vi) { return ia3::ball_slot(vi); }
extern "C" int ia3cpu_ball_lane(int vi) { return ia3::ball_lane(vi); }
extern "C" int ia3cpu_ball_vi(int lane, int slot) { return ia3::ball_vi(lane, slot); }
extern "C" int ia3cpu_in_ball(int oz, int ox, int oy, int r) { return ia3::in_ball(oz, ox, oy, r) ? 1 : 0; }
extern "C" void ia3cpu_ball_limits(int* out) { out[0] = ia3::BALL_LANES; out[1] = ia3::BALL_SLOTS; out[2] = ia3::BALL_MAXVOX; }

extern "C" float ia3cpu_npsum_f32(const float* a, int n) { return ia3::np_sum<float>(a, n); }
extern "C" double ia3cpu_npsum_f64(const double* a, int n) { return ia3::np_sum<double>(a, n); }

// gfit_fast: vals n float64 copies of the values, coords (3, n) ints; the steps and their order are moments_from_lds'
extern "C" void ia3cpu_ff_moments(const double* vals, const int* coords, int n, int kind, double bk_f, double* out) {
  if (n == 0) { for (int k = 0; k < 12; ++k) out[k] = __builtin_nan(""); return; }
  const int k = (int)((double)n * bk_f);
  double bk = 0.0;
  for (int e = 0; e < n; ++e)
    if (ia3::ff_is_kth(vals, n, e, k)) bk = vals[e];
  std::vector<double> wn((size_t)n);
  const double h = ia3::ff_weights(vals, n, bk, kind, wn.data());
  const int* x[3] = {coords, coords + n, coords + 2 * (size_t)n};
  double c[3];
  for (int a = 0; a < 3; ++a) c[a] = ia3::ff_centroid(x[a], wn.data(), n);
  out[0] = h; out[1] = c[0]; out[2] = c[1]; out[3] = c[2]; out[4] = bk;
  const int ii[6] = {0, 1, 2, 0, 0, 1}, jj[6] = {0, 1, 2, 1, 2, 2};
  for (int q = 0; q < 6; ++q) out[5 + q] = ia3::ff_cov(x[ii[q]], c[ii[q]], x[jj[q]], c[jj[q]], wn.data(), n);
  out[11] = __builtin_nan("");
}

// own[v] = 1 when offset v (n_off x 3) of seed i's ball stays with seed i against the seeds js[0..m) (ascending, i left out)
extern "C" void ia3cpu_ff_owner(const double* centres, int i, const int* js, int m, const int* off, int n_off,
                                unsigned char* own) {
  for (int v = 0; v < n_off; ++v) {
    own[v] = 1;
    for (int q = 0; q < m; ++q) {
      const int j = js[q];
      if (ia3::ff_loses(centres[3 * j] - centres[3 * i], centres[3 * j + 1] - centres[3 * i + 1],
                        centres[3 * j + 2] - centres[3 * i + 2], off[3 * v], off[3 * v + 1], off[3 * v + 2], j < i))
        own[v] = 0;
    }
  }
}
