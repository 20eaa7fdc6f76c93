// The background test of the lazy seed detector (seed.hip: bg_sparse3_k, bg_sparse_k), for host and device.
//
// A first-stage candidate is a seed when  minimum_filter(min_im) != min_im  and  max_im - min_im >= th  at its voxel
// (fitting.py:102-125).  With the 27 values m[q] of min_im around it (q = 9 dz + 3 dx + dy, centre q = 13), cmin = m[13]
// and diff = float32(cmax) - float32(cmin), the sequential form of the test is
//     vmin = cmin;  for q = 0..26: vmin = m[q] < vmin ? m[q] : vmin;      accept iff vmin != cmin && (double)diff >= th.
// vmin only ever falls from cmin, and it falls at the first m[q] < vmin; while it has not fallen, vmin == cmin, so it
// falls at all exactly when some m[q] < cmin.  Hence vmin != cmin <=> (exists q: m[q] < cmin), except for cmin = NaN:
// there no compare is true, vmin stays NaN and vmin != cmin holds, but diff = cmax - NaN = NaN fails the threshold test,
// so the candidate is rejected either way.  (-0.0 < +0.0 is false in both forms; a NaN neighbour is never below anything
// in both forms; +-inf compare as numbers.)  The test is therefore the same predicate as
//     reject  if !((double)diff >= th)                              -- the centre value alone
//     accept  if one of the 8 in-plane neighbours is < cmin         -- plane z alone
//     else    accept iff one of the 18 values of planes z - 1, z + 1 is < cmin
// and the two outer planes, two thirds of what the sparse pass gathers, are needed only by a candidate that passes the
// threshold and is an in-plane 3 x 3 minimum (ties included) of a smooth background: hardly any.
//
// Arithmetic as in the sequential form: diff in float32, the threshold compare in double, neighbour compares in float32.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define IA3_BG_HD __host__ __device__ inline
#else
#define IA3_BG_HD inline
#endif

namespace ia3bg {

enum { BG_REJECT = 0, BG_ACCEPT = 1, BG_OUTER = 2 };

// Centre step: m9 = the nine values of plane z (index 3 dx + dy, centre 4).  *diff is set whatever the answer.
IA3_BG_HD int centre_step(const float* m9, float cmax, double th_low, float* diff) {
  const float cmin = m9[4];
  const float d = cmax - cmin;   // float32(max_im) - float32(min_im), fitting.py:106
  *diff = d;
  if (!((double)d >= th_low)) return BG_REJECT;
  bool below = false;
  for (int q = 0; q < 9; ++q) below = below || (m9[q] < cmin);
  return below ? BG_ACCEPT : BG_OUTER;
}

// Full step: m27 = all 27 values (index 9 dz + 3 dx + dy, centre 13).  *diff is set whatever the answer.
IA3_BG_HD bool full_step(const float* m27, float cmax, double th_low, float* diff) {
  const float cmin = m27[13];
  const float d = cmax - cmin;
  *diff = d;
  if (!((double)d >= th_low)) return false;
  bool below = false;
  for (int q = 0; q < 27; ++q) below = below || (m27[q] < cmin);
  return below;
}

}  // namespace ia3bg
