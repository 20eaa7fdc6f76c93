// The column-in-registers axis-0 kernel (device code only: compiled by hipcc through gauss_col.inc, one translation unit per
// dtype and stack depth, and by hiprtc at run time for depths without one, gauss_col_dispatch.hip).  Needs
// ia3_gauss_dev.h and ia3k::DOG_PAIR_ZGROUPS.
namespace ia3colk {
using namespace ia3g;

// ---- axis 0 of a long filter on a short stack: the whole column in registers, border folded into the weights ----
// With Z <= 64 planes and R = 30 most taps of an output land on the reflected (or clamped) border, i.e. on a plane
// the sum already holds: out[z] = sum_p W[z][p] * in[p] with W[z][p] = the taps that map to plane p added up
// (host, f64).  Both border modes give W[Z-1-z][Z-1-p] = W[z][p], so the mirror outputs z and zz = Z-1-z are
//   a = sum_p W[z][p] v[p],  b = sum_p W[z][p] v[Z-1-p]:
// the same weights on the same PAIRS of inputs.  With H = Z / 2, E[q] = v[q] + v[Z-1-q], O[q] = v[q] - v[Z-1-q] (formed
// once per column, as the planes arrive in mirror pairs) and Wp, Wm = (W[z][q] +- W[z][Z-1-q]) / 2 (host, f64):
//   P = sum_q Wp[z][q] E[q],  M = sum_q Wm[z][q] O[q],  a = P + M,  b = P - M
// — Z fused multiply-adds and two additions per pair of outputs, where the sums above take 2 * (31 .. Z) (84 on average
// at Z = 50) and NI_Correlate1D's sequence 2 * (3R + 1).  An odd depth keeps its centre plane: it enters P with its own
// weight, and the centre row has M = 0 and one output.  wf = the stream of ia3_col_weights.h (uniform, compile-time
// offsets -> scalar loads).
//
// The order of operations is not NI_Correlate1D's, so this is a certified path like the fused one (ia3_gauss_dev.h).
// u = 2^-53; data and taps non-negative; n = (Z+1)/2 terms in the P chain (H in the M chain); tw = roundings in one
// W[z][p] (host sums of up to tw + 1 non-negative taps: relative error <= tw u).  First order in u throughout, one
// unit added at the end for the second-order terms (all factors below are < 2^10).
//   E^ = (v + v')(1 + e1), O^ = (v - v')(1 + e2), |e| <= u, and |O^| <= E^ (rounding is monotone).
//   Wp^ = Wp (1 + t), |t| <= (tw + 1) u;  |Wm^ - Wm| <= (tw + 1) u Wp;  |Wm^| <= Wp^.
//   A chain of n terms (one product, n - 1 FMAs) returns sum_q w_q x_q (1 + g_q), |g_q| <= n u.  All terms of P are
//   non-negative: |P^ - P| <= (n + tw + 2) u P.  The terms of M are bounded one by one by those of P:
//   |M^ - M| <= n u P + (tw + 2) u P.
//   a^ = fl(P^ + M^):  |a^ - a| <= (2n + 2 tw + 4) u P + u a <= (2n + 2 tw + 5) u P, since a <= 2 P; the same for b.
//   With the second-order unit:  |a^ - a|, |b^ - b| <= C u P,  C = 2n + 2 tw + 6,  P = (a + b) / 2.
// THE BOUND IS RELATIVE TO P, NOT TO a: a column that is zero in one half and 6e4 in the other has a << b, and its a^
// is thousands of ulps of a away from a.  Hence
//   (i)  a pair with |M^| > (1 - 1/K) P^, K = 4 (i.e. min(a^, b^) < P^ / K) takes the reference sequence for both outputs;
//   (ii) elsewhere P <= K a^ (1 + (n + tw + 7) u), so |a^ - a| <= K C ulp(a^) + 1 (ulp(x) >= u x), and NI_Correlate1D's own
//        sum r (3R + 1 roundings on non-negative terms) has |r - a| <= (3R + 1) u a <= (3R + 2) ulp(a^): the float32 /
//        uint16 value of a^ can differ from that of r only when a^ lies within K C + 3R + 3 f64 ulps of a float32 rounding
//        midpoint / an integer.  The default guard is K C + 3R + 4 (ia3_col_weights.h: col_guard; 326 for Z = 50, R = 30,
//        'reflect'), and `uncertain` measures in units of at least one ulp.
// Those outputs (about 1.2e-6 of them at the default guard), and every output of a thread that saw a sign bit, are
// recomputed with the reference sequence from global memory.
//
// RF > 0 (the short pass, below) needs the raw column back, exactly.  It gets the DOUBLED column, 2 v[q] = E + O and
// 2 v[Z-1-q] = E - O, in place and without a multiplication, and the short filter's taps HALVED (ftaps, host): a factor
// of two passes through every rounding of NI_Correlate1D's sequence, so the bits are those of the plain sequence.  The
// two values are exact iff E and O were formed without rounding.  uint16: always.  float32: the sum and the difference
// of two non-negative values whose exponent fields are at most 28 apart (or one of which is zero) fit in 53 bits.  A sticky
// test on the raw bits decides per thread: unsigned maximum of the bits, unsigned minimum of bits - 1 (zeros wrap to
// the top and drop out), exponent fields of the two at most 28 apart and no inf / nan.  A thread that fails it is treated
// like one that saw a sign bit: reference sequence for the whole column, and its wave takes the short pass from memory.
constexpr int COL_K = 4;   // rule (i) of the header (ia3_col_weights.h: COL_LOPSIDED_K)
template <int Z> constexpr int eo_len() { return (Z / 2) * Z + ((Z & 1) ? (Z + 1) / 2 : 0); }

// order-preserving integer key of a stored value and back (strip maxima of the short pass, below)
template <class T> __device__ __forceinline__ int mx_key(T q);
template <> __device__ __forceinline__ int mx_key<float>(float q) { const int b = (int)__float_as_uint(q); return b ^ ((b >> 31) & 0x7fffffff); }
template <> __device__ __forceinline__ int mx_key<uint16_t>(uint16_t q) { return (int)q; }
template <class T> __device__ __forceinline__ float mx_val(int k);
template <> __device__ __forceinline__ float mx_val<float>(int k) { return __uint_as_float((unsigned)(k ^ ((k >> 31) & 0x7fffffff))); }
template <> __device__ __forceinline__ float mx_val<uint16_t>(int k) { return (float)k; }

// one plane of the strip maxima of the short pass (see the kernel; planes come in z order)
template <class T, int Z>
__device__ __forceinline__ void strip_max(int z, T qf, int& keep, unsigned lane15, bool mx_row, float* __restrict__ smx, unsigned mx_base) {
#define IA3_DPP(v, c) __builtin_amdgcn_update_dpp(0, (v), (c), 0xf, 0xf, true)
  int k = mx_key<T>(qf), t;
  t = IA3_DPP(k, 0x128); k = k > t ? k : t;   // row_ror:8
  t = IA3_DPP(k, 0x124); k = k > t ? k : t;
  t = IA3_DPP(k, 0x122); k = k > t ? k : t;
  t = IA3_DPP(k, 0x121); k = k > t ? k : t;
  t = IA3_DPP(k, 0x142); k = k > t ? k : t;   // row_bcast15 (the lower row reads 0: its lanes are not used)
#undef IA3_DPP
  keep = lane15 == (unsigned)(z & 15) ? k : keep;
  if ((z & 15) == 15 || z == Z - 1) {
    if (mx_row) smx[mx_base + (unsigned)(z & ~15)] = mx_val<T>(keep);
  }
}

// RF > 0: the same launch also runs the axis-0 pass of a SHORT filter (radius RF, 'reflect' border) over the column
// it holds and writes it to fout — the DoG seed detector filters one stack with a short and a long kernel, and the
// two first passes share every load (NI_Correlate1D's sequence, unfused: the short pass is not a certified path).
// ftaps = the short filter's taps times 0.5 (see the header).
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
  // the column as mirror pairs: e[q] = v[q] + v[Z-1-q], o[q] = v[q] - v[Z-1-q]; an odd depth's centre plane is e[H], raw
  constexpr int H = Z / 2, NP = (Z + 1) / 2;
  double e[NP], o[H];
  unsigned bmax = 0u, bmin = ~0u;   // float32: unsigned max of the raw bits (sign bit seen <=> top bit set), min of bits - 1
  auto track = [&](T t) {
    if constexpr (sizeof(T) == 4) {
      const unsigned u = sign_of<T>(t);
      bmax = bmax > u ? bmax : u;
      if constexpr (RF > 0) { const unsigned m = u - 1u; bmin = bmin < m ? bmin : m; }
    }
  };
#pragma unroll
  for (int q = 0; q < H; ++q) {
    const T t0 = buf_ld<T>(rin, voff, (unsigned)q * pbytes), t1 = buf_ld<T>(rin, voff, (unsigned)(Z - 1 - q) * pbytes);
    track(t0); track(t1);
    const double d0 = (double)t0, d1 = (double)t1;
    e[q] = d0 + d1;
    o[q] = d0 - d1;
  }
  if constexpr (Z & 1) {
    const T t = buf_ld<T>(rin, voff, (unsigned)H * pbytes);
    track(t);
    e[H] = (double)t;
  }
  bool bad = (int)bmax < 0;   // a sign bit, or (RF > 0) a pair that did not add up exactly: see the header
  if constexpr (RF > 0 && sizeof(T) == 4) {
    const unsigned emax = bmax >> 23, emin = (bmin + 1u) >> 23;   // bmin + 1: the smallest non-zero bits, 0 for a column of zeros
    bad = bad || emax - emin > 28u || emax == 255u;
  }
  const bool wave_bad = RF > 0 && __builtin_amdgcn_ballot_w64(bad) != 0ull;   // (uniform)
  unsigned long long redo = 0;   // outputs that need NI_Correlate1D's own sequence (about one thread in 1.6e4 has one)
  const bool all = cert < 0 || bad;
  if (all) redo = Z == 64 ? ~0ull : (1ull << Z) - 1;
  if (!all) {
    // the weight stream is read in pieces of CH doubles (scalar loads), the next piece in flight while this one is
    // used; the scheduling barrier keeps the compiler from hoisting every load to the top (and spilling SGPRs)
    constexpr int N = eo_len<Z>(), CH = 8, NC = (N + CH - 1) / CH;
    double P = 0.0, M = 0.0;
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
          constexpr int z = i / Z < H ? i / Z : H, zz = Z - 1 - z, k = i - z * Z;   // row (z == H: the centre row of an odd depth)
          constexpr bool centre_row = z == H;
          constexpr int q = centre_row ? k : k >> 1;
          constexpr bool minus = !centre_row && (k & 1) != 0 && q < H;
          constexpr bool last = centre_row ? k == NP - 1 : k == Z - 1;
          const double w = cur[i - c * CH];
          if constexpr (minus) {
            if constexpr (q == 0) M = o[0] * w; else M = __builtin_fma(o[q], w, M);
          } else {
            if constexpr (q == 0) P = e[0] * w; else P = __builtin_fma(e[q], w, P);
          }
          if constexpr (last && centre_row) {
            if (uncertain<T>(P, cert)) redo |= 1ull << z;
            const T qa = cvt<T>(P);
            buf_st<T>(qa, rout, voff, (unsigned)z * pbytes);
            if constexpr (RF > 0) note(z * NGZ / Z, qa);
          } else if constexpr (last) {
            const double a = P + M, b = P - M;
            const bool lopsided = __builtin_fabs(M) > P * (1.0 - 1.0 / COL_K);   // rule (i); false for P = M = 0, nan is caught by `uncertain`
            if (uncertain<T>(a, cert) || lopsided) redo |= 1ull << z;
            const T qa = cvt<T>(a);
            buf_st<T>(qa, rout, voff, (unsigned)z * pbytes);
            if constexpr (RF > 0) note(z * NGZ / Z, qa);
            if (uncertain<T>(b, cert) || lopsided) redo |= 1ull << zz;
            const T qb = cvt<T>(b);
            buf_st<T>(qb, rout, voff, (unsigned)zz * pbytes);
            if constexpr (RF > 0) note(zz * NGZ / Z, qb);
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
  // per SIMD instead of four, +0.1 ms).  It works on the doubled column, made in place from the pairs (header; multiplying
  // the sums by 0.5 instead made the compiler keep a second, sliding copy of the column: 139 registers, three waves).
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
    // (a wave with a thread whose pairs are not exact takes the whole short pass from memory, at the end of the kernel)
    if (!wave_bad) {
#pragma unroll
      for (int q = 0; q < H; ++q) {
        e[q] = e[q] + o[q];                      // 2 v[q]
        o[q] = __builtin_fma(o[q], -2.0, e[q]);  // 2 v[q] - 2 O = 2 v[Z-1-q]: representable, so the fused result is exact
        if ((q & 3) == 3) __builtin_amdgcn_sched_barrier(0);
      }
      if constexpr (Z & 1) e[H] = e[H] + e[H];   // the centre plane of an odd depth
      __builtin_amdgcn_sched_barrier(0);
      auto frow =[&](auto zc) -> bool {
        constexpr int z = decltype(zc)::value;
        auto val = [&](int i) -> double { return i < NP ? e[i] : o[Z - 1 - i]; };   // (compile-time index)
        double acc = val(z) * ftaps.w[0];
#pragma unroll
        for (int j = RF; j >= 1; --j) {
          const int lo = z - j < 0 ? -(z - j) - 1 : z - j, hi = z + j >= Z ? 2 * Z - 1 - (z + j) : z + j;   // compile-time
          acc = acc + (val(lo) + val(hi)) * ftaps.w[j];
        }
        const T qf = cvt<T>(acc);
        buf_st<T>(qf, rf, voff, (unsigned)z * pbytes);
        if (want_mx) strip_max<T, Z>(z, qf, keep, lane15, mx_row, smx, mx_base);
        return true;
      };
      static_for_until<0, Z>(frow);
      __builtin_amdgcn_sched_barrier(0);
    }
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
  // The short pass of a wave with a thread whose pairs were not exact (never on real images): from memory, in a rolled
  // loop like the tail above, for all its lanes — the reference sequence is the definition, so that is right for every
  // lane, and the strip maxima see all 32 stored values.  Here, behind everything else, it costs the kernel no register.
  if constexpr (RF > 0) {
    if (wave_bad) {
      constexpr unsigned ZP = (Z + 15) & ~15;
      const bool mx_row = (threadIdx.x & 16) != 0, want_mx = smx != nullptr;
      const unsigned lane15 = threadIdx.x & 15, mx_base = (p >> 5) * ZP + lane15;
      int keep = 0;
#pragma unroll 1
      for (int z = 0; z < Z; ++z) {
        T lo[RF], hi[RF];
#pragma unroll
        for (int j = 1; j <= RF; ++j) {
          lo[j - 1] = in[(size_t)border_idx(z - j, Z, IA3_MODE_REFLECT) * plane + p];
          hi[j - 1] = in[(size_t)border_idx(z + j, Z, IA3_MODE_REFLECT) * plane + p];
        }
        double acc = (ld<T>(in, (size_t)z * plane + p) * 2.0) * ftaps.w[0];
#pragma unroll
        for (int j = RF; j >= 1; --j) acc = acc + (((double)lo[j - 1] + (double)hi[j - 1]) * 2.0) * ftaps.w[j];
        const T qf = cvt<T>(acc);
        fout[(size_t)z * plane + p] = qf;
        if (want_mx) strip_max<T, Z>(z, qf, keep, lane15, mx_row, smx, mx_base);
      }
    }
  }
}

}  // namespace ia3colk
