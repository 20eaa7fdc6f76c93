// TEST INFRASTRUCTURE — host build of the product's LM core (csrc/ia3_lm.h) driven the way the paired driver of
// csrc/fit.hip drives it: two fits on the same voxels, each with a solver state and a work area of its own, their
// evaluations alternating and each fit stopping when its own state says so.  Every fit is also run on its own through
// lm_solve; the caller compares the two bit for bit.  Not shipped, not a fallback.
#include <algorithm>
#include <cstring>
#include <vector>
#include <cmath>
#include "../../imageanalysis3_amd/csrc/ia3_lm.h"
#include "../../imageanalysis3_amd/csrc/ia3_init.h"

using namespace ia3;

namespace {
struct CpuEval {   // as tests/native/lm_cpu.cpp
  const float* im; const double* cz; const double* cx; const double* cy; int n; FitCfg cfg;
  int zero_diag_first = -1;   // exactly-zero diagonal entries of JᵀJ at the first evaluation
  double eval(const double* x, double* A, double* g) {
    Geom gm; make_geom(x, cfg, gm);
    double ss = 0;
    int nbad = 0;
    for (int k = 0; k < NTRI; ++k) A[k] = 0;
    for (int k = 0; k < NP; ++k) g[k] = 0;
    for (int v = 0; v < n; ++v) {
      double J[NP];
      double F = model_jac(gm, cz[v], cx[v], cy[v], J);
      double r = (gm.ebk_f + F) - (double)im[v];
      if (r != r) nbad += 2; else if (r - r != 0.0) nbad += 1;
      ss += r * r;
      for (int i = 0; i < NP; ++i) { g[i] += J[i] * r; for (int j = i; j < NP; ++j) A[tri(i, j)] += J[i] * J[j]; }
    }
    if (zero_diag_first < 0) {
      zero_diag_first = 0;
      for (int j = 0; j < NP; ++j) zero_diag_first += A[tri(j, j)] == 0.0;
    }
    if (nbad >= 2) return NAN;
    return sqrt(ss);
  }
};

struct Fit {   // one fit's own: nothing here is shared with the other fit of the pair
  CpuEval ev;
  LMWork w;
  LMState s;
  int maxfev;
  bool want;
};

void put(const LMWork& w, int info, int nfev, int iter, double fnorm, int zero_diag, double* out) {
  for (int k = 0; k < NP; ++k) out[k] = w.x[k];
  out[10] = fnorm; out[11] = info; out[12] = nfev; out[13] = iter; out[14] = zero_diag;
}
}  // namespace

// Two fits (index 0, 1) on the voxels (vals, coords): delta[f], kind[f], maxfev[f]; variant / iw3 as FitCfg.  The start
// point comes from the ten smallest / largest of lohi (n_lohi >= 10 values: the whole ball, also where the fits see fewer
// voxels).  out: 4 x 15 doubles — fit 0 alone, fit 1 alone, fit 0 interleaved, fit 1 interleaved — each x[10], fnorm,
// info, nfev, iter, zero diagonal entries of JᵀJ at the start.  order: which fit is evaluated first in a round.
extern "C" int ia3cpu_pair(const double* vals, const int* coords, int n, const double* lohi, int n_lohi,
                           const double* center, const double* delta, const int* kind, const int* maxfev, int variant,
                           const double* iw3, int order, double* out) {
  if (n_lohi < 10 || n < 1) return 1;
  std::vector<float> im(n); std::vector<double> cz(n), cx(n), cy(n), sorted(lohi, lohi + n_lohi);
  for (int v = 0; v < n; ++v) { im[v] = (float)vals[v]; cz[v] = coords[3 * v]; cx[v] = coords[3 * v + 1]; cy[v] = coords[3 * v + 2]; }
  std::sort(sorted.begin(), sorted.end());
  const double ftol = 1.49012e-8, xtol = 1.49012e-8, gtol = 0.0, factor = 100.0;
  Fit f[2];
  for (int pass = 0; pass < 2; ++pass) {   // 0: each fit alone through lm_solve; 1: interleaved through lm_advance
    for (int k = 0; k < 2; ++k) {
      CpuEval& ev = f[k].ev;
      ev.im = im.data(); ev.cz = cz.data(); ev.cx = cx.data(); ev.cy = cy.data(); ev.n = n;
      ev.zero_diag_first = -1;
      if (variant == 1) { ev.cfg.min_ws = 0.25; ev.cfg.max_ws = 16.0; }
      else { ev.cfg.min_ws = 0.5 * 0.5; ev.cfg.max_ws = 4.0 * 4.0; }
      ev.cfg.delta = delta[k]; ev.cfg.init_w = 1.5; ev.cfg.variant = variant;
      for (int a = 0; a < 3; ++a) { ev.cfg.c0[a] = center[a]; ev.cfg.iw[a] = variant == 1 ? iw3[a] : 0.0; }
      std::memset(&f[k].w, 0xA5, sizeof(LMWork));   // a work area full of junk: whatever is read was written by this fit
      init_guess(sorted.data(), sorted.data() + n_lohi - 10, kind[k], ev.cfg, f[k].w.x);
      f[k].maxfev = maxfev[k];
    }
    if (pass == 0) {
      for (int k = 0; k < 2; ++k) {
        LMResult r = lm_solve(f[k].ev, f[k].w, ftol, xtol, gtol, f[k].maxfev, factor);
        put(f[k].w, r.info, r.nfev, r.iter, r.fnorm, f[k].ev.zero_diag_first, out + 15 * k);
      }
    } else {
      for (int k = 0; k < 2; ++k) { lm_begin(f[k].s); f[k].want = true; }
      int rounds = 0;
      while (f[0].want || f[1].want) {
        double fn[2] = {0.0, 0.0};
        for (int q = 0; q < 2; ++q) {   // the evaluations of a round, one fit after the other
          const int k = order ? 1 - q : q;
          if (f[k].want) fn[k] = f[k].ev.eval(lm_eval_x(f[k].s, f[k].w), lm_eval_A(f[k].s, f[k].w), lm_eval_g(f[k].s, f[k].w));
        }
        for (int q = 0; q < 2; ++q) {   // the algebra of a round (on the device: both at once, a half-wave each)
          const int k = order ? q : 1 - q;
          if (f[k].want) f[k].want = lm_advance(f[k].s, f[k].w, fn[k], ftol, xtol, gtol, f[k].maxfev, factor);
        }
        if (++rounds > 100000) return 2;
      }
      for (int k = 0; k < 2; ++k)
        put(f[k].w, f[k].s.info, f[k].s.nfev, f[k].s.iter, f[k].s.fnorm, f[k].ev.zero_diag_first, out + 15 * (2 + k));
    }
  }
  return 0;
}
