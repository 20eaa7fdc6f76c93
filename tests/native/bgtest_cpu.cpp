// CPU check of the two-step background test of the sparse seed pass (csrc/ia3_bgtest.h) for tests/test_bg_order_cpu.py:
// the centre step followed, on need, by the full step must give the answer (and the height) of the sequential loop the
// kernels ran before, on random 27-tuples with many ties, on float32 and uint16-quantised values, on an exhaustive sweep
// of special values and on thresholds at either side of diff.  Stand-alone: prints its counts, returns 0 when all agree.
#include "../../imageanalysis3_amd/csrc/ia3_bgtest.h"
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

// the sequential form (bg_sparse_k before the centre-first order): vmin scan over all 27 values
static bool sequential(const float* mval, float cmax, double th_low, float* diff_out) {
  const float cmin = mval[13];
  float vmin = cmin;
  for (int q = 0; q < 27; ++q) vmin = mval[q] < vmin ? mval[q] : vmin;
  const float diff = cmax - cmin;
  *diff_out = diff;
  return vmin != cmin && (double)diff >= th_low;
}

// the kernels' order: centre plane, then everything; *outer = the outer planes were needed
static bool two_step(const float* mval, float cmax, double th_low, float* diff_out, bool* outer) {
  const int v = ia3bg::centre_step(mval + 9, cmax, th_low, diff_out);
  *outer = v == ia3bg::BG_OUTER;
  if (v != ia3bg::BG_OUTER) return v == ia3bg::BG_ACCEPT;
  return ia3bg::full_step(mval, cmax, th_low, diff_out);
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {   // xorshift64*
  rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
  return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}

static long long n_cases = 0, n_bad = 0, n_outer = 0, n_accept = 0;

static void check(const float* m, float cmax, double th) {
  float d0, d1, d2;
  bool outer;
  const bool a = sequential(m, cmax, th, &d0);
  const bool b = two_step(m, cmax, th, &d1, &outer);
  const bool c = ia3bg::full_step(m, cmax, th, &d2);   // what the kernels do with the early decision switched off
  ++n_cases;
  n_outer += outer;
  n_accept += a;
  bool same = a == b && a == c;
  if (a) same = same && std::memcmp(&d0, &d1, 4) == 0 && std::memcmp(&d0, &d2, 4) == 0;   // the height of an accepted seed, on the bits
  if (!same) {
    if (n_bad < 10) {
      std::printf("MISMATCH seq %d two-step %d full %d cmax %a th %a:", (int)a, (int)b, (int)c, cmax, th);
      for (int q = 0; q < 27; ++q) std::printf(" %a", m[q]);
      std::printf("\n");
    }
    ++n_bad;
  }
}

// thresholds on either side of diff (and at it), and cmax = NaN
static void check_thresholds(const float* m, float cmax) {
  const float diff = cmax - m[13];
  const double d = (double)diff;
  const double ths[] = {d, std::nextafter(d, -INFINITY), std::nextafter(d, INFINITY), (double)std::nextafterf(diff, -INFINITY),
                        (double)std::nextafterf(diff, INFINITY), 0.0, -1.0, 540.0, (double)NAN, (double)INFINITY, -(double)INFINITY};
  for (double th : ths) check(m, cmax, th);
  check(m, NAN, 540.0);
  check(m, NAN, -(double)INFINITY);
}

int main() {
  float m[27];
  // ---- random tuples from few distinct values: float32 ----
  const float lv[] = {399.25f, 399.5f, 400.0f, 400.0f, 400.0f, 400.125f, 401.0f, -3.5f};
  for (int n = 0; n < 500000; ++n) {
    const int nl = 1 + (int)(rnd() % 8);
    for (int q = 0; q < 27; ++q) m[q] = lv[rnd() % nl];
    const float cmax = (rnd() & 1) ? 940.0f + (float)(rnd() % 5) * 0.125f : lv[rnd() % 8] + (float)(rnd() % 1200);
    const float diff = cmax - m[13];
    const double th = (rnd() % 3 == 0) ? (double)diff : ((rnd() & 1) ? 540.0 : (double)std::nextafterf(diff, (rnd() & 1) ? INFINITY : -INFINITY));
    check(m, cmax, th);
  }
  // ---- random tuples, uint16-quantised values ----
  for (int n = 0; n < 500000; ++n) {
    const int span = 1 + (int)(rnd() % 3);
    const int base = (rnd() & 1) ? 400 : (int)(rnd() % 65534);
    for (int q = 0; q < 27; ++q) { int v = base + (int)(rnd() % span); m[q] = (float)(uint16_t)(v > 65535 ? 65535 : v); }
    const float cmax = (float)(uint16_t)(rnd() % 65536);
    const float diff = cmax - m[13];
    const double th = (rnd() % 3 == 0) ? (double)diff : ((rnd() & 1) ? 540.0 : (double)diff + ((rnd() & 1) ? 1.0 : -1.0));
    check(m, cmax, th);
  }
  const long long n_random = n_cases, outer_random = n_outer;
  // ---- exhaustive: special values at the centre, at one in-plane and at one out-of-plane position ----
  const float sp[] = {NAN, -INFINITY, INFINITY, -0.0f, 0.0f, 400.0f, 412.5f};
  const float fill[] = {400.0f, 412.5f, 0.0f, -0.0f, INFINITY, -INFINITY, NAN};
  const int inpl[] = {9, 12, 14, 17}, outpl[] = {0, 4, 8, 18, 22, 26};
  const float cmaxs[] = {1000.0f, 400.0f, 0.0f, -0.0f, INFINITY, -INFINITY, NAN};
  for (float f : fill)
    for (float c : sp)
      for (float a : sp)
        for (float b : sp)
          for (int ip : inpl)
            for (int op : outpl)
              for (float cmax : cmaxs) {
                for (int q = 0; q < 27; ++q) m[q] = f;
                m[13] = c; m[ip] = a; m[op] = b;
                check_thresholds(m, cmax);
              }
  std::printf("cases %lld (random %lld, outer planes needed %lld of them), accepted %lld, outer in all %lld, mismatches %lld\n",
              n_cases, n_random, outer_random, n_accept, n_outer, n_bad);
  // the inputs must exercise all three answers of the centre step
  if (n_outer == 0 || n_outer == n_cases || n_accept == 0) { std::printf("degenerate inputs\n"); return 2; }
  return n_bad ? 1 : 0;
}
