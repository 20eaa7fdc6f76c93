// Column-in-registers axis-0 pass (see the comment at the kernel).  Compiled once per dtype and stack depth (gauss_col_one.hip
// with -DIA3_COL_F32=0/1 -DIA3_COL_Z=<depth>, Makefile: FOLD_DEPTHS): the kernels are long straight-line code, ~7 s each,
// and the translation units build in parallel.
#include "ia3_gauss.h"
#include "ia3_col_weights.h"
#include <unistd.h>
#include <cstring>
#include <mutex>
#include <vector>

using namespace ia3g;

#include "gauss_col_kernel.inc"
using namespace ia3colk;

namespace {

// weight stream of gauss_axis0_folded (ia3_col_weights.h), cached on the device per (Z, R, mode, taps)
struct FoldKey { int Z, R, mode; std::vector<double> w; };
struct FoldEntry { FoldKey k; double* d = nullptr; };
std::mutex g_fold_mu;
std::vector<FoldEntry> g_fold;
pid_t g_fold_pid = 0;
int g_fold_dev = -1;

template <int Z, int R>
const double* folded_rows(const Taps& t, int mode, hipStream_t s) {
  std::lock_guard<std::mutex> g(g_fold_mu);
  {   // tables of another process (fork) or another device are not ours: start over
    int dev = -1;
    (void)hipGetDevice(&dev);
    if (g_fold_pid != getpid() || g_fold_dev != dev) { g_fold.clear(); g_fold_pid = getpid(); g_fold_dev = dev; }
  }
  for (auto& e : g_fold)
    if (e.k.Z == Z && e.k.R == R && e.k.mode == mode && std::memcmp(e.k.w.data(), t.w, (R + 1) * sizeof(double)) == 0) return e.d;
  const std::vector<double> rows = col_evenodd_rows(Z, R, mode, t.w);
  FoldEntry e;
  e.k = FoldKey{Z, R, mode, std::vector<double>(t.w, t.w + R + 1)};
  if (hipMalloc((void**)&e.d, rows.size() * sizeof(double)) != hipSuccess) return nullptr;
  // a blocking copy, once per filter: the table must be in place before any stream uses the cached pointer
  if (hipMemcpy(e.d, rows.data(), rows.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(e.d); return nullptr; }
  (void)s;
  if (g_fold.size() >= 16) { g_fold.erase(g_fold.begin()); }   // the evicted table stays allocated: launches may be in flight
  g_fold.push_back(e);
  return e.d;
}

template <class T, int Z, int R>
int run_folded(const T* src, size_t plane, const Taps& t, int mode, T* dst, hipStream_t s, int cert) {
  const double* wf = folded_rows<Z, R>(t, mode, s);
  if (!wf) return ia3rt::set_error(IA3_ENOMEM, "folded weight table");
  hipLaunchKernelGGL((gauss_axis0_folded<T, Z, R, 0>), dim3((unsigned)((plane + 255) / 256)), dim3(256), 0, s, src, dst, plane, wf, t, mode, cert,
                     (T*)nullptr, t, (float*)nullptr, (float*)nullptr, 0, (float*)nullptr);
  return 0;
}

// both first passes of the DoG pair in one launch (long: folded, -> dst; short: radius RF, reflect, -> fdst)
template <class T, int Z, int R, int RF>
int run_folded_pair(const T* src, size_t plane, const Taps& t, T* dst, const Taps& ft, T* fdst, hipStream_t s, int cert,
                    float* smin, float* sabs, int Y, float* smx) {
  const double* wf = folded_rows<Z, R>(t, IA3_MODE_REFLECT, s);
  if (!wf) return ia3rt::set_error(IA3_ENOMEM, "folded weight table");
  hipLaunchKernelGGL((gauss_axis0_folded<T, Z, R, RF>), dim3((unsigned)((plane + 255) / 256)), dim3(256), 0, s, src, dst, plane, wf, t,
                     (int)IA3_MODE_REFLECT, cert, fdst, ft, smin, sabs, Y, smx);
  return 0;
}


}  // namespace

#define IA3_CAT2(a, b) a##b
#define IA3_CAT(a, b) IA3_CAT2(a, b)
#define IA3_CAT3(a, b, c) IA3_CAT(IA3_CAT(a, b), c)

namespace ia3g {

// entry points of this (dtype, depth): folded_axis0_<dtype>_z<Z>, folded_pair_<dtype>_z<Z> (gauss_col_dispatch.hip picks by depth)
int IA3_CAT3(folded_axis0, IA3_COL_SUFFIX, IA3_CAT(_z, IA3_COL_Z))(const IA3_COL_T* src, size_t plane, const Taps& t, int mode, IA3_COL_T* dst,
                                                                    hipStream_t s, int cert) {
  return run_folded<IA3_COL_T, IA3_COL_Z, 30>(src, plane, t, mode, dst, s, cert);
}

int IA3_CAT3(folded_pair, IA3_COL_SUFFIX, IA3_CAT(_z, IA3_COL_Z))(const IA3_COL_T* src, size_t plane, const Taps& bt, IA3_COL_T* dst, const Taps& ft,
                                                                  IA3_COL_T* fdst, hipStream_t s, int cert, float* smin, float* sabs, int Y, float* smx) {
  return run_folded_pair<IA3_COL_T, IA3_COL_Z, 30, 3>(src, plane, bt, dst, ft, fdst, s, cert, smin, sabs, Y, smx);
}

}  // namespace ia3g
