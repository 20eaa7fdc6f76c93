// The column-in-registers axis-0 kernel (device code only: compiled by hipcc through gauss_col.inc, one translation unit per
// dtype and stack depth, and by hiprtc at run time for depths without one, gauss_col_dispatch.hip).  Needs
// ia3_gauss_dev.h and ia3k::DOG_PAIR_ZGROUPS.
namespace ia3colk {
using namespace ia3g;

// ---- axis 0 of a long filter on a short stack: the whole column in registers, border folded into the weights ----
// With Z <= 64 planes and R = 30 most taps of an output land on the reflected (or clamped) border, i.e. on a plane
// the sum already holds: out[z] = sum_p W[z][p] * in[p] with W[z][p] = the taps that map to plane p added up
// (host, f64), p in [max(0, z-R), min(Z-1, z+R)].  That is 31..Z fused multiply-adds per output instead of R pair
// additions + R+1 multiply-adds (Z = 50: 42 on average against 66 with the 6-wide chunks), every input is read
// once, and the rows of z and Z-1-z share their weights (W[Z-1-z][Z-1-p] = W[z][p]).  The order of operations is
// not NI_Correlate1D's, so this is a certified path like the fused one above: for non-negative data and taps both
// sums are within (3R+1) resp. (Z+2) * 2^-53 * S of the exact sum S, so the float32 / uint16 value can only differ
// when the folded sum lies within 3R+Z+3 f64 ulps of a quantisation boundary.  Those outputs, and every output of
// a thread that saw a sign bit, are recomputed with the reference sequence from global memory.  wf = the folded
// rows 0 .. (Z-1)/2 packed one after the other (uniform, compile-time offsets -> scalar loads).
template <int Z, int R> constexpr int fold_lo(int z) { return z - R > 0 ? z - R : 0; }
template <int Z, int R> constexpr int fold_hi(int z) { return z + R < Z - 1 ? z + R : Z - 1; }
template <int Z, int R> constexpr int fold_off(int z) {
  int o = 0;
  for (int i = 0; i < z; ++i) o += fold_hi<Z, R>(i) - fold_lo<Z, R>(i) + 1;
  return o;
}
// flat position i of the packed weight stream -> its row, and the row offsets, as tables built once per (Z, R) (the
// kernel asks for them at every one of its ~Z^2 / 2 compile-time positions)
template <int Z, int R> struct FoldTab {
  static constexpr int H = (Z + 1) / 2, N = fold_off<Z, R>((Z + 1) / 2);
  int off[H + 1];
  int row[N];
  constexpr FoldTab() : off(), row() {
    int o = 0;
    for (int z = 0; z < H; ++z) {
      off[z] = o;
      const int n = fold_hi<Z, R>(z) - fold_lo<Z, R>(z) + 1;
      for (int k = 0; k < n; ++k) row[o + k] = z;
      o += n;
    }
    off[H] = o;
  }
};
template <int Z, int R> inline constexpr FoldTab<Z, R> fold_tab{};

// order-preserving integer key of a stored value and back (strip maxima of the short pass, below)
template <class T> __device__ __forceinline__ int mx_key(T q);
template <> __device__ __forceinline__ int mx_key<float>(float q) { const int b = (int)__float_as_uint(q); return b ^ ((b >> 31) & 0x7fffffff); }
template <> __device__ __forceinline__ int mx_key<uint16_t>(uint16_t q) { return (int)q; }
template <class T> __device__ __forceinline__ float mx_val(int k);
template <> __device__ __forceinline__ float mx_val<float>(int k) { return __uint_as_float((unsigned)(k ^ ((k >> 31) & 0x7fffffff))); }
template <> __device__ __forceinline__ float mx_val<uint16_t>(int k) { return (float)k; }

// RF > 0: the same launch also runs the axis-0 pass of a SHORT filter (radius RF, 'reflect' border) over the column
// it holds and writes it to fout — the DoG seed detector filters one stack with a short and a long kernel, and the
// two first passes share every load (NI_Correlate1D's sequence, unfused: the short pass is not a certified path).
template <class T, int Z, int R, int RF>
__global__ __launch_bounds__(256) void gauss_axis0_folded(const T* __restrict__ in, T* __restrict__ out, size_t plane,
                                                          const double* __restrict__ wf, Taps taps, int mode, int cert,
                                                          T* __restrict__ fout, Taps ftaps,
                                                          float* __restrict__ smin, float* __restrict__ sabs, int Y,
                                                          float* __restrict__ smx) {
  // addressing: buffer descriptors, this thread's 32-bit byte offset in the plane + the plane's byte offset as the
  // scalar operand (the host checks Z * plane * sizeof(T) < 2^31): no vector address arithmetic per access
  const unsigned p = blockIdx.x * 256u + threadIdx.x;
  if (p >= plane) return;
  const unsigned voff = p * (unsigned)sizeof(T), pbytes = (unsigned)plane * (unsigned)sizeof(T);
  const int nbytes = (int)((unsigned)Z * pbytes);
  const __amdgpu_buffer_rsrc_t rin = __builtin_amdgcn_make_buffer_rsrc((void*)in, (short)0, nbytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rout = __builtin_amdgcn_make_buffer_rsrc((void*)out, (short)0, nbytes, 0x00020000);
  // smin / sabs (optional; the seed detector's lazy background filter): smallest value and largest magnitude of this
  // launch's long-filter output per group of planes (NGZ groups), row and 32-column strip — the block minima the
  // detector's bound is made from, taken from the registers instead of a pass over the stored stack.  The folded value of
  // an output that is recomputed below may differ from the stored one by a float32 ulp / one count: the bound's slack
  // covers it (seed.hip).
  constexpr int NGZ = ia3k::DOG_PAIR_ZGROUPS;
  float gmin[NGZ], gabs[NGZ];   // of the quantised outputs (uint16: magnitudes are not needed, the slack is a constant)
#pragma unroll
  for (int g = 0; g < NGZ; ++g) { gmin[g] = __builtin_huge_valf(); gabs[g] = 0.f; }
  auto note = [&](int g, T q) {
    const float f = (float)q;
    gmin[g] = fminf(gmin[g], f);
    if constexpr (sizeof(T) == 4) gabs[g] = fmaxf(gabs[g], fabsf(f));
  };
  double v[Z];
  unsigned sbits = 0;
#pragma unroll
  for (int z = 0; z < Z; ++z) {
    const T t = buf_ld<T>(rin, voff, (unsigned)z * pbytes);
    sbits |= sign_of<T>(t);
    v[z] = (double)t;
  }
  unsigned long long redo = 0;   // outputs that need NI_Correlate1D's own sequence (about one thread in 3e4 has one)
  const bool all = cert < 0 || (int)sbits < 0;
  if (all) redo = Z == 64 ? ~0ull : (1ull << Z) - 1;
  if (!all) {
    // the weight stream is read in pieces of CH doubles (scalar loads), the next piece in flight while this one is
    // used; the scheduling barrier keeps the compiler from hoisting every load to the top (and spilling SGPRs)
    constexpr int N = FoldTab<Z, R>::N, CH = 8, NC = (N + CH - 1) / CH;
    double a = 0.0, b = 0.0;
    double cur[CH], nxt[CH];
#pragma unroll
    for (int i = 0; i < CH; ++i) nxt[i] = wf[i];   // the table is padded to a multiple of CH
    auto piece = [&](auto cc) -> bool {
      constexpr int c = decltype(cc)::value;
#pragma unroll
      for (int i = 0; i < CH; ++i) cur[i] = nxt[i];
      if constexpr (c + 1 < NC) {
#pragma unroll
        for (int i = 0; i < CH; ++i) nxt[i] = wf[(c + 1) * CH + i];
      }
      auto tap = [&](auto ic) -> bool {
        constexpr int i = c * CH + decltype(ic)::value;
        if constexpr (i < N) {
          constexpr int z = fold_tab<Z, R>.row[i], zz = Z - 1 - z, lo = fold_lo<Z, R>(z), k = i - fold_tab<Z, R>.off[z];
          constexpr bool last = i + 1 == fold_tab<Z, R>.off[z + 1];
          const double w = cur[i - c * CH];
          if constexpr (k == 0) {
            a = v[lo] * w;
            if constexpr (zz != z) b = v[Z - 1 - lo] * w;
          } else {
            a = __builtin_fma(v[lo + k], w, a);
            if constexpr (zz != z) b = __builtin_fma(v[Z - 1 - lo - k], w, b);
          }
          if constexpr (last) {
            if (uncertain<T>(a, cert)) redo |= 1ull << z;
            const T qa = cvt<T>(a);
            buf_st<T>(qa, rout, voff, (unsigned)z * pbytes);
            if constexpr (RF > 0) note(z * NGZ / Z, qa);
            if constexpr (zz != z) {
              if (uncertain<T>(b, cert)) redo |= 1ull << zz;
              const T qb = cvt<T>(b);
              buf_st<T>(qb, rout, voff, (unsigned)zz * pbytes);
              if constexpr (RF > 0) note(zz * NGZ / Z, qb);
            }
          }
        }
        return true;
      };
      static_for_until<0, CH>(tap);
      __builtin_amdgcn_sched_barrier(0);
      return true;
    };
    static_for_until<0, NC>(piece);
  }
  // The short pass runs BEHIND the long one: here no load is in flight, so the raw values no longer sit beside the column
  // of doubles (in front of the long pass the strip maxima below took the kernel from 123 to 164 registers, three waves
  // per SIMD instead of four, +0.1 ms; here it needs 124).
  if constexpr (RF > 0) {
    static_assert(Z > RF, "single reflection");
    const __amdgpu_buffer_rsrc_t rf = __builtin_amdgcn_make_buffer_rsrc((void*)fout, (short)0, nbytes, 0x00020000);
    // smx (optional, with smin; the seed detector skips planes by it, ia3_seedskip.h): the largest STORED value of this
    // short pass per plane, row and 32-column strip, [row][strip][plane, padded to ZP] floats.  The reduction runs on an
    // order-preserving integer key (mx_key: integer max instructions take the lane rotations as DPP operands and need no
    // NaN canonicalisation; fmaxf on rotated copies came to 25 instructions a plane and 164 registers against 123).  A
    // NaN with the sign bit clear orders above +inf and comes out as NaN: the reader takes a NaN strip for +inf (live);
    // one with the sign bit set orders below -inf and is left out, as fmaxf would.  32 lanes = two DPP rows: four
    // rotations inside each row, then lane 15 of the lower row into the upper one (row_bcast15): every lane of the upper
    // row holds the strip's maximum.  Lane 16 + k keeps that of plane 16 g + k, and the row stores 16 planes at once, in
    // whole 64-byte pieces.
    constexpr unsigned ZP = (Z + 15) & ~15;
    const bool mx_row = (threadIdx.x & 16) != 0;
    const unsigned lane15 = threadIdx.x & 15;
    const unsigned mx_base = (p >> 5) * ZP + lane15;   // Y % 32 == 0: strip (row, column / 32) is p / 32; ZP * plane / 32 < 2^31
    int keep = 0;
    const bool want_mx = smx != nullptr;   // (uniform)
    auto frow = [&](auto zc) -> bool {
      constexpr int z = decltype(zc)::value;
      double acc = v[z] * ftaps.w[0];
#pragma unroll
      for (int j = RF; j >= 1; --j) {
        const int lo = z - j < 0 ? -(z - j) - 1 : z - j, hi = z + j >= Z ? 2 * Z - 1 - (z + j) : z + j;   // compile-time
        acc = acc + (v[lo] + v[hi]) * ftaps.w[j];
      }
      const T qf = cvt<T>(acc);
      buf_st<T>(qf, rf, voff, (unsigned)z * pbytes);
      if (want_mx) {
#define IA3_DPP(v, c) __builtin_amdgcn_update_dpp(0, (v), (c), 0xf, 0xf, true)
        int k = mx_key<T>(qf), o;
        o = IA3_DPP(k, 0x128); k = k > o ? k : o;   // row_ror:8
        o = IA3_DPP(k, 0x124); k = k > o ? k : o;
        o = IA3_DPP(k, 0x122); k = k > o ? k : o;
        o = IA3_DPP(k, 0x121); k = k > o ? k : o;
        o = IA3_DPP(k, 0x142); k = k > o ? k : o;   // row_bcast15 (the lower row reads 0: its lanes are not used)
#undef IA3_DPP
        keep = lane15 == (unsigned)(z & 15) ? k : keep;
        if constexpr ((z & 15) == 15 || z == Z - 1) {
          if (mx_row) smx[mx_base + (z & ~15)] = mx_val<T>(keep);
        }
      }
      // two planes at a time: left alone, the scheduler interleaves all Z planes and the kernel comes to 339 registers
      return true;
    };
    static_for_until<0, Z>(frow);
    __builtin_amdgcn_sched_barrier(0);
  }

  // NI_Correlate1D's own sequence, inputs re-read (a few outputs per 10^7 on non-negative data)
  // NI_Correlate1D's own sequence, inputs re-read from memory, all 2R+1 loads of an output in flight together
  while (redo) {
    const int z = __builtin_ctzll(redo);
    redo &= redo - 1;
    T lo[R], hi[R];
#pragma unroll
    for (int j = 1; j <= R; ++j) {
      lo[j - 1] = in[(size_t)border_idx(z - j, Z, mode) * plane + p];
      hi[j - 1] = in[(size_t)border_idx(z + j, Z, mode) * plane + p];
    }
    double acc = ld<T>(in, (size_t)z * plane + p) * taps.w[0];
#pragma unroll
    for (int j = R; j >= 1; --j) acc = acc + ((double)lo[j - 1] + (double)hi[j - 1]) * taps.w[j];
    const T qr = cvt<T>(acc);
    out[(size_t)z * plane + p] = qr;
    if constexpr (RF > 0) {
      const int g = z * NGZ / Z;
#pragma unroll
      for (int k = 0; k < NGZ; ++k)
        if (k == g) note(k, qr);
    }
  }
  if (RF > 0 && smin) {   // Y % 32 == 0 (host): 32 consecutive lanes are 32 consecutive columns of one row
    float fmn[NGZ], fab[NGZ];
#pragma unroll
    for (int g = 0; g < NGZ; ++g) {
      fmn[g] = gmin[g];
      fab[g] = gabs[g];
      // 32 lanes = two DPP rows: four rotations inside each row (fused into the min / max instructions), one exchange between them
#define IA3_ROR(v, c) __uint_as_float(__builtin_amdgcn_update_dpp(0, __float_as_uint(v), 0x120 | (c), 0xf, 0xf, false))
      fmn[g] = fminf(fmn[g], IA3_ROR(fmn[g], 8)); fab[g] = fmaxf(fab[g], IA3_ROR(fab[g], 8));
      fmn[g] = fminf(fmn[g], IA3_ROR(fmn[g], 4)); fab[g] = fmaxf(fab[g], IA3_ROR(fab[g], 4));
      fmn[g] = fminf(fmn[g], IA3_ROR(fmn[g], 2)); fab[g] = fmaxf(fab[g], IA3_ROR(fab[g], 2));
      fmn[g] = fminf(fmn[g], IA3_ROR(fmn[g], 1)); fab[g] = fmaxf(fab[g], IA3_ROR(fab[g], 1));
#undef IA3_ROR
      fmn[g] = fminf(fmn[g], __shfl_xor(fmn[g], 16));
      fab[g] = fmaxf(fab[g], __shfl_xor(fab[g], 16));
    }
    if ((threadIdx.x & 31) == 0) {
      const unsigned x = p / (unsigned)Y, yb = (p % (unsigned)Y) >> 5;
      const size_t rows = plane / (unsigned)Y, nby = (unsigned)Y >> 5;
#pragma unroll
      for (int g = 0; g < NGZ; ++g) {
        smin[((size_t)g * rows + x) * nby + yb] = fmn[g];
        sabs[((size_t)g * rows + x) * nby + yb] = fab[g];
      }
    }
  }
}

}  // namespace ia3colk
