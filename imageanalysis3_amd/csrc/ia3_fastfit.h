// Arithmetic of the closed-form moment fit gfit_fast (External/Fitting_v4.py:433-458) and of the Voronoi ownership
// test of fast_fit_big_image (:513-518), one operation at a time in the order NumPy / SciPy perform them.
//
// Host/device agnostic: fastfit.hip runs these on a few lanes of the wave that gathered the voxels (from LDS);
// tests/native/fastfit_cpu.cpp builds them with g++ for the CPU test against the reference's own rows.
// Voxel values arrive as float64 copies of the image's values (exact for float32 and uint16); `kind` says which
// arithmetic NumPy uses for the weights (the codes of ia3_gaussfit_voxels):
//   kind 0: float32 image -> float32 subtract, clip at 0, float32 pairwise sum, float32 divide
//   kind 1: uint16 image  -> uint16 subtract (wraps; `weights < 0` never holds), exact integer sum, float64 divide
//   kind 2: float64 image -> float64 throughout
#pragma once
#include <stdint.h>
#include "ia3_npsum.h"

namespace ia3 {

constexpr int FF_MAXVOX = NPSUM_MAX;   // voxels of one moment fit (ball of radius_fit <= 5: 512 offsets)

// scipy.spatial.distance.cdist(..., 'euclidean') of one pair in float64: differences, squares added in axis order, sqrt.
// c = (another centre) - (this centre), o = integer voxel offset from this centre's truncated position.
IA3_HD double ff_cdist(double c0, double c1, double c2, int o0, int o1, int o2) {
  const double d0 = c0 - (double)o0, d1 = c1 - (double)o1, d2 = c2 - (double)o2;
  double s = 0.0;
  s = s + d0 * d0;
  s = s + d1 * d1;
  s = s + d2 * d2;
  return sqrt(s);
}

// Voronoi ownership (:516-518): does the offset o of this seed's ball go to seed j instead?  rel = centre_j - centre_i;
// argmin over the ascending neighbour list takes the first minimum, so an equal distance goes to the lower index.
IA3_HD bool ff_loses(double rel0, double rel1, double rel2, int o0, int o1, int o2, bool j_before_i) {
  const double dme = ff_cdist(0.0, 0.0, 0.0, o0, o1, o2);
  const double dj = ff_cdist(rel0, rel1, rel2, o0, o1, o2);
  return dj < dme || (dj == dme && j_before_i);
}

// np.sort(v)[k] by rank counting: is element e the k-th smallest (any of a run of equal values qualifies)?
template <class P>
IA3_HD bool ff_is_kth(P v, int n, int e, int k) {
  const double ve = v[e];
  int less = 0, equal = 0;
  for (int j = 0; j < n; ++j) {
    const double vj = v[j];
    less += vj < ve ? 1 : 0;
    equal += vj == ve ? 1 : 0;
  }
  return less <= k && k < less + equal;
}

// weights = v - bk (clipped at 0 where the dtype is signed), h = max(weights), weights / sum(weights): wn[e] holds the
// normalised weight as the float64 NumPy multiplies the coordinates with.  Returns h.
template <class P, class Q>
IA3_HD double ff_weights(P v, int n, double bk, int kind, Q wn) {
  if (kind == 0) {
    const float b = (float)bk;
    float h = 0.0f;
    for (int e = 0; e < n; ++e) {
      float w = (float)v[e] - b;
      if (w < 0.0f) w = 0.0f;
      wn[e] = (double)w;
      if (e == 0 || w > h) h = w;
    }
    const float s = np_sum_f<float>([&](int i) { return (float)wn[i]; }, n);
    for (int e = 0; e < n; ++e) wn[e] = (double)((float)wn[e] / s);
    return (double)h;
  }
  if (kind == 1) {
    const unsigned b = (unsigned)bk;
    unsigned h = 0;
    unsigned long long s = 0;
    for (int e = 0; e < n; ++e) {
      const unsigned w = ((unsigned)v[e] - b) & 0xffffu;
      wn[e] = (double)w;
      if (w > h) h = w;
      s += w;
    }
    const double sd = (double)s;
    for (int e = 0; e < n; ++e) wn[e] = wn[e] / sd;
    return (double)h;
  }
  double h = 0.0;
  for (int e = 0; e < n; ++e) {
    double w = v[e] - bk;
    if (w < 0.0) w = 0.0;
    wn[e] = w;
    if (e == 0 || w > h) h = w;
  }
  const double s = np_sum_f<double>([&](int i) { return (double)wn[i]; }, n);
  for (int e = 0; e < n; ++e) wn[e] = wn[e] / s;
  return h;
}

// np.sum(X_ * weights, -1)[a]: integer coordinate times float64 weight, summed in NumPy's order
template <class X, class Q>
IA3_HD double ff_centroid(X xa, Q wn, int n) {
  return np_sum_f<double>([&](int i) { return (double)xa[i] * (double)wn[i]; }, n);
}

// np.sum(X_c[:, i] * X_c[:, j] * weights, -1) with X_c = X_.T - centroid
template <class X, class Q>
IA3_HD double ff_cov(X xi, double ci, X xj, double cj, Q wn, int n) {
  return np_sum_f<double>([&](int e) { return (((double)xi[e] - ci) * ((double)xj[e] - cj)) * (double)wn[e]; }, n);
}

}  // namespace ia3
