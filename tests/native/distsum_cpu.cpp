// CPU check of the host/device arithmetic of the population distance summaries (csrc/ia3_distsum.h) for
// tests/test_distance_summary_cpu.py:
//   ia3_dist_qstar against the literal `sqrt(q) <= th` over random thresholds, at q* and its neighbours, and at the edges;
//   the digit passes of the radix select (ds_matches, ds_digit, ds_pick_bin over parts and bins as median_k walks them,
//   ds_upper_key, ds_median) against a sort, on values with ties, zeros, inf, NaN and neighbouring doubles;
//   ds_pairwise on a fixed series, printed for the test to compare with np.add.reduce.
// Stand-alone: prints its counts, returns 0 when all agree.
#include "../../imageanalysis3_amd/csrc/ia3_distsum.h"
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

using namespace ia3ds;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd64() {   // xorshift64*
  rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
  return rng_state * 0x2545F4914F6CDD1Dull;
}
static double uniform() { return (double)(rnd64() >> 11) / 9007199254740992.0; }

static long long n_th = 0, n_q = 0, n_sel = 0, n_bad = 0;

static bool literal(double q, double th) { volatile double r = std::sqrt(q); return r <= th; }

static void check_th(double th) {
  const double qs = ia3_dist_qstar(th);
  ++n_th;
  if (!(th >= 0)) { n_bad += qs >= 0; return; }
  if (th == INFINITY) { n_bad += qs != INFINITY; return; }
  if (!literal(qs, th)) ++n_bad;
  const double up = std::nextafter(qs, INFINITY);
  if (up != INFINITY && literal(up, th)) ++n_bad;
  // the predicate on q* and neighbours, and on random q around the threshold
  double q = qs;
  for (int i = 0; i < 3 && q > 0; ++i) q = std::nextafter(q, -INFINITY);
  for (int i = 0; i < 7; ++i, q = std::nextafter(q, INFINITY), ++n_q)
    if (literal(q, th) != (q <= qs)) ++n_bad;
  for (int i = 0; i < 4; ++i, ++n_q) {
    const double r = th * th * (0.5 + uniform());
    if (literal(r, th) != (r <= qs)) ++n_bad;
  }
}

// the select as median_k runs it: NS parts of DS_BINS / NS bins each, the digit passes ended once the rank is alone in its bin
static double select_median(const std::vector<double>& q, int NS, bool early) {
  const int PER = DS_BINS / NS;
  u64 prefix = DS_TOP;
  unsigned k = 0, c = 0;
  std::vector<unsigned> hist(DS_BINS), part(NS);
  int last = DS_PASSES - 1;
  for (int pass = 0; pass < DS_PASSES; ++pass) {
    std::fill(hist.begin(), hist.end(), 0u);
    for (double v : q) {
      if (v != v) continue;
      const u64 key = ds_key(v);
      if (ds_matches(key, prefix, pass)) ++hist[ds_digit(key, pass)];
    }
    for (int s = 0; s < NS; ++s) {
      part[s] = 0;
      for (int b = s * PER; b < (s + 1) * PER; ++b) part[s] += hist[b];
    }
    if (pass == 0) {
      c = 0;
      for (int s = 0; s < NS; ++s) c += part[s];
      k = c ? (c - 1) / 2 : 0;
    }
    bool more = false;
    if (c) {
      const int p = ds_pick_bin(part.data(), 0, NS, k);
      const int b = ds_pick_bin(hist.data(), p * PER, PER, k);
      prefix |= (u64)b << ds_shift(pass);
      more = hist[b] > 1;
    }
    if (!more && early) { last = pass; break; }   // alone in its bin: the last pass reads the value off
  }
  const int low = ds_shift(last);
  unsigned le = 0;
  u64 mn = ~0ull, lo = 0;
  for (double v : q) {
    if (v != v) continue;
    const u64 key = ds_key(v), top = key >> low;
    if (top <= prefix >> low) {
      ++le;
      if (top == prefix >> low) lo = key > lo ? key : lo;
    } else if (key < mn) mn = key;
  }
  return ds_median(c, lo, ds_upper_key(lo, c, le, mn));
}

static double sorted_median(std::vector<double> q) {
  std::vector<double> v;
  for (double x : q) if (x == x) v.push_back(x);
  if (v.empty()) return NAN;
  std::sort(v.begin(), v.end());
  const size_t c = v.size();
  volatile double lo = std::sqrt(v[(c - 1) / 2]), hi = std::sqrt(v[c / 2]);
  if (c & 1) return lo;
  volatile double sum = lo + hi;
  return sum / 2.0;
}

static void check_select(const std::vector<double>& q) {
  const double want = sorted_median(q);
  for (int NS : {4, 16, 64})
    for (bool early : {true, false}) {   // a tile ends its digit passes early only when all of its entries can
      const double got = select_median(q, NS, early);
      ++n_sel;
      if (want != want ? got == got : memcmp(&got, &want, 8) != 0) ++n_bad;
    }
}

int main() {
  // thresholds
  for (double th : {0.0, -0.0, 0.5, 0.6, 1.0, 3.0, 500.0, 1e-200, 1e-160, 4.9e-324, 1e154, 1.3407807929942596e154, 1e200,
                    std::numeric_limits<double>::max(), (double)INFINITY, -1.0, -(double)INFINITY, (double)NAN})
    check_th(th);
  for (int i = 0; i < 200000; ++i) check_th(uniform() * 2000.0);
  for (int i = 0; i < 20000; ++i) check_th(std::ldexp(0.5 + uniform(), (int)(rnd64() % 1200) - 600));
  if (ia3_dist_qstar(-1.0) >= 0 || ia3_dist_qstar(NAN) >= 0 || ia3_dist_qstar(INFINITY) != INFINITY || ia3_dist_qstar(-0.0) != 0) ++n_bad;
  // the select
  for (int N : {1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 129, 601, 2000})
    for (int kind = 0; kind < 8; ++kind)
      for (int rep = 0; rep < (N < 100 ? 40 : 6); ++rep) {
        std::vector<double> q(N);
        const double base = 1.0e6 + uniform();
        for (double& v : q) {
          switch (kind) {
            case 0: v = uniform() * 1.0e6; break;                                    // plain
            case 1: v = (double)(rnd64() % 4); break;                               // ties and zeros
            case 2: { v = base; for (int s = (int)(rnd64() % 6); s > 0; --s) v = std::nextafter(v, INFINITY); } break;   // neighbours
            case 3: v = rnd64() % 5 == 0 ? INFINITY : uniform(); break;              // inf
            case 4: v = std::ldexp(uniform(), (int)(rnd64() % 2000) - 1040); break;  // every exponent, subnormals
            case 5: v = rnd64() % 3 == 0 ? NAN : uniform() * 10.0; break;            // NaNs
            case 6: v = rnd64() % 2 ? NAN : (double)(rnd64() % 2); break;            // NaNs and ties
            default: v = NAN; break;                                                 // no value
          }
          if (kind < 5 && rnd64() % 10 == 0) v = NAN;
        }
        check_select(q);
      }
  printf("thresholds %lld, predicates %lld, selects %lld, mismatches %lld\n", n_th, n_q, n_sel, n_bad);
  // pairwise sums of v[i] = (i * 2654435761 mod 2^32) / 2^32 * 3000
  for (long long N : {1LL, 7LL, 8LL, 9LL, 128LL, 129LL, 136LL, 641LL, 5000LL, 100003LL}) {
    const double s = ds_pairwise([](long long i) { return (double)((uint64_t)i * 2654435761ull % 4294967296ull) / 4294967296.0 * 3000.0; }, N);
    uint64_t bits;
    memcpy(&bits, &s, 8);
    printf("pairwise %lld %016llx\n", N, (unsigned long long)bits);
  }
  return n_bad ? 1 : 0;
}
