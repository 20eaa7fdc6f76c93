// CPU build of the plane-skipping certificate of the fused seed detector (csrc/ia3_seedskip.h) for
// tests/test_seed_skip_certificate_cpu.py.  Compile with -ffp-contract=off, as the library is.
#include "../../imageanalysis3_amd/csrc/ia3_seedskip.h"

extern "C" {

// taps w[0..3], centre first; 1 and *sup when skipping is allowed, 0 when the taps are refused
int skip_taps_sup(const double* w, double* sup) { return ia3skip::taps_sup(w, sup) ? 1 : 0; }

// certified upper bound of max_im for n window maxima
void skip_front_bound(const float* m, int n, double sup, int u16, double* out) {
  for (int i = 0; i < n; ++i) out[i] = u16 ? ia3skip::front_bound<true>(m[i], sup) : ia3skip::front_bound<false>(m[i], sup);
}

int skip_unit_live(double ubound, double bound, double th_test) { return ia3skip::unit_live(ubound, bound, th_test) ? 1 : 0; }

}
