/* ia3.h — C ABI of libia3.so: MI355X-native kernels for ImageAnalysis3's per-FOV spot-calling path.
 *
 * The reference has no FFI on this path (pure Python); these entry points are what
 * thin ctypes shims carrying the reference's dotted names bind.  Each entry cites the reference
 * interface it replaces (paths relative to the reference tree).
 *
 * Conventions
 *   - stacks are C-order (Z, X, Y) ("z, x, y" = array axes 0,1,2), dtype IA3_U16 or IA3_F32;
 *   - host pointers are borrowed for the duration of the call; outputs are caller-allocated;
 *   - every function returns 0 on success or a negative IA3_E* code; ia3_last_error() gives
 *     the message of the last failure on the calling thread;
 *   - device state is created lazily by the first call in a process (safe after fork);
 *   - `ia3_stack` handles keep a stack resident in HBM so filter -> seed -> fit chain without
 *     host round trips;
 *   - threads and streams: every host thread that calls the library gets HIP streams of its own; `_dev` entry
 *     points queue their kernels on the calling thread's stream and may return before they have run, calls of one
 *     thread execute in the order they were made, and anything that returns data to the host (downloads, seed and
 *     spot tables, drifts) waits for what it needs.  A resident stack is handed to ANOTHER host thread only after
 *     ia3_sync() on the thread that produced it; ia3_fit_fovs, which works on threads of its own, orders them after
 *     the calling thread's stream by itself.
 */
#ifndef IA3_H
#define IA3_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IA3_U16 0
#define IA3_F32 1

#define IA3_OK 0
#define IA3_EINVAL (-1)   /* bad argument (shim raises ValueError / IndexError as the reference does) */
#define IA3_EHIP (-2)     /* HIP runtime / kernel failure */
#define IA3_ENOMEM (-3)
#define IA3_ECAPACITY (-4) /* caller-provided output buffer too small; *n_out holds the needed size */
#define IA3_EUNSUPPORTED (-5)

#define IA3_MODE_REFLECT 0  /* scipy.ndimage 'reflect' (half-sample symmetric) */
#define IA3_MODE_NEAREST 1  /* scipy.ndimage 'nearest' (edge replicate) */
#define IA3_MODE_CONSTANT 2 /* map_coordinates 'constant' (cval) */

typedef struct ia3_stack ia3_stack;

/* ---- runtime ------------------------------------------------------------------------------- */
int ia3_init(int device);                 /* select device (default: LOCAL_RANK or 0); idempotent */
const char* ia3_last_error(void);
const char* ia3_version(void);
int ia3_device_name(char* buf, int len);
int ia3_sync(void);                       /* hipStreamSynchronize on the library stream */
void* ia3_stream(void);                   /* hipStream_t the kernels are launched on */
int ia3_release_workspace(void);          /* drop cached device scratch buffers */
/* The long Gaussian passes of get_seeds keep a whole z column in registers, one kernel per stack depth: the library is
   built with the depths of FOLD_DEPTHS (25 30 33 35 40 45 50 60), any other depth from 16 to 64 planes is compiled at run
   time (hiprtc: ~35 s once per depth, dtype and machine, kept in IA3_RTC_CACHE or <library dir>/_rtc; IA3_RTC=0 turns it
   off) the first time it is used.  This call does that ahead of time.  Returns 1 = built in, 2 = compiled at run time (or
   taken from the cache), 0 = not available (the sliding-window kernels run: same results, slower), < 0 = error.  The
   reference takes any single_im_size (io_tools/load.py:166-180). */
int ia3_prepare_depth(int dtype, int Z);
/* The column kernel's host side, for its tests (no device needed).  ia3_col_guard: the default guard distance (f64 ulps)
   of its certificate for a stack depth, a radius and a border mode.  ia3_col_weights: its weight stream for the taps
   w[0 .. R] (csrc/ia3_col_weights.h); writes at most cap doubles and returns the stream's length. */
int ia3_col_guard(int Z, int R, int mode);
int ia3_col_weights(int Z, int R, int mode, const double* taps, double* out, int cap);
/* the scratch cache: out6 = {idle bytes, bytes in use, blocks, hipMalloc calls, hipFree calls, ms spent in both} since
   the library was loaded; a steady-state loop adds no calls (each hipFree synchronises the device) */
int ia3_workspace_stats(double* out6);
/* the fused seed detector's (tile, plane) units of the calling thread's last get_seeds: out2 = {units filtered and tested,
   units in all}; {0, 0} when that call did not run the fused detector (see IA3_TUNE_SEED_SKIP) */
int ia3_seed_skip_stats(double* out2);
/* the sparse background pass of the calling thread's last get_seeds: out2 = {first-stage candidates it tested, those of
   them for which it evaluated the planes z - 1 and z + 1}; {0, 0} when that call ran the dense filter (see
   IA3_TUNE_SEED_BGORDER) */
int ia3_seed_bg_stats(double* out2);
/* per-kernel timing with HIP events on the library stream (off by default) */
int ia3_profile_enable(int on);
int ia3_profile_collect(char* buf, int len); /* "kernel,count,total_ms\n" lines since last collect */
/* Test / tuning knobs; results never depend on them.  IA3_TUNE_GAUSS_CERT: guard distance (f64 ulps) of the
 * certified fused-multiply-add path of the long Gaussian passes; -2 default (4R+8), -1 path off (always the
 * reference operation sequence), large values send every output through the reference sequence after the check. */
#define IA3_TUNE_GAUSS_CERT 1
/* IA3_TUNE_DFT_VALU: 1 = the upsampled-DFT contractions of the phase correlation run on the vector unit (first
 * version) instead of the f64 matrix cores; shifts agree to rounding. */
#define IA3_TUNE_DFT_VALU 2
/* IA3_TUNE_UPLOAD_THREADS: helper threads that copy a host array into the pinned staging ring of ia3_stack_upload
 * (environment IA3_UPLOAD_THREADS); 0 (default: it measured fastest, 56 GB/s) = one plain hipMemcpyAsync from
 * pageable memory. */
#define IA3_TUNE_UPLOAD_THREADS 3
/* IA3_TUNE_SEED_DENSE: 1 = get_seeds always runs all three passes of the background filter on the whole stack; 0
 * (default) = the lazy form: the axis-0 pass everywhere, the other two only around candidate maxima (seed.hip).  Seeds
 * are identical either way. */
#define IA3_TUNE_SEED_DENSE 4
/* IA3_TUNE_FIT_NBLIST: longest per-seed neighbour list the fit kernel reads (default and maximum 64); seeds with more
 * overlapping neighbours scan the seed list instead — same neighbours in the same order.  Tests lower it to drive
 * ordinary fields through the scan. */
#define IA3_TUNE_FIT_NBLIST 5
/* IA3_TUNE_FFT_C2C: 1 = the phase correlation transforms the (real) stacks with complex-to-complex FFTs (first
 * version); 0 (default) = real-input transforms on half spectra.  Shifts agree to rounding. */
#define IA3_TUNE_FFT_C2C 6
/* IA3_TUNE_FIT_FUSE: 1 (default) = in ia3_fit_run a seed whose ball overlaps no other seed's gets its first fit and
 * sweep 1 from ONE wavefront (same voxels, gathered once; one hand-over); 0 = two work-list positions as for every other
 * seed.  Tables are identical bit for bit. */
#define IA3_TUNE_FIT_FUSE 7
/* IA3_TUNE_GAUSS_FOLD: 1 (default) = the axis-0 pass of a long filter (radius >= 16) over a stack of 30, 40 or 50
 * planes holds the column in registers and folds the border into the weights (certified like the fused path, same
 * fallback); 0 = the sliding-window pass for every depth.  Results are identical bit for bit. */
#define IA3_TUNE_GAUSS_FOLD 8
/* IA3_TUNE_SEED_STRIPS: 1 (default) = where the column kernel of IA3_TUNE_GAUSS_FOLD runs for the seed detector and the
 * row length is a multiple of 32, the lower bound of the lazy background filter is made from minima that kernel takes from
 * its registers (per group of planes, row and 32 columns); 0 = from a pass over the stored axis-0 result (per plane).  Only
 * the number of first-stage candidates can differ, never a seed. */
#define IA3_TUNE_SEED_STRIPS 9
/* IA3_TUNE_FIT_WAVES: persistent wavefronts of the fit kernel per SIMD, 1 or 2 (default 2: the kernel is built for 256
 * registers).  Tables are identical bit for bit. */
#define IA3_TUNE_FIT_WAVES 10
/* IA3_TUNE_FIT_MERGE: 1 (default) = once the first launch (first fits + sweep 1) has left fewer than 1 seed in 64
 * unconverged, all remaining sweeps go out in one launch, ordered by the work list's dependencies alone (a seed's
 * sweep k+1 no longer waits for the slowest fit of sweep k anywhere in the batch); 0 = two sweeps per launch throughout.
 * Tables are identical bit for bit. */
#define IA3_TUNE_FIT_MERGE 11
/* IA3_TUNE_WARP_ONEPASS: the cubic warp's spline prefilter along the two long axes.  64 (default) = every sample read
 * once and written once: the anticausal recursion of a tile starts from a value certified by two bounding chains over
 * the samples behind it (warp.hip), with the two-sweep recursion over the rest of the line where the chains do not
 * meet; 1..63 = the same with that many warm-up samples (tests: short warm-ups fail often and drive lines through the
 * fallback); 0 = two sweeps over whole lines; -1 = two sweeps and the one-output-per-thread gather.  Results are
 * identical bit for bit. */
#define IA3_TUNE_WARP_ONEPASS 12
/* IA3_TUNE_FIT_KDQ: entries of the per-voxel queue of the Voronoi tie queries on the device (1..24, default 24); a query
 * that needs more is finished on the host with the same tree (tests lower it to drive fields through that path).  Tables
 * are identical bit for bit. */
#define IA3_TUNE_FIT_KDQ 13
/* IA3_TUNE_FIT_MEMO: 1 (default) = a repeat sweep does not run a refit whose inputs — the image ball and the records of
 * the overlapping seeds — are what they were at the seed's previous refit: the fit would return the same row and the
 * seed is marked converged, as the reference's loop does after repeating it (External/Fitting_v4.py:651-680); 0 = every
 * refit is run.  Tables and sweep counts are identical bit for bit; the evaluation counters count the fits that ran. */
#define IA3_TUNE_FIT_MEMO 14
/* IA3_TUNE_SEED_FUSED: 1 (default) = where get_seeds pairs the two axis-0 passes in one column kernel (short filter of
 * radius 3, background radius 30, a folded stack depth), one kernel runs the short filter's axis-1 and axis-2 passes and
 * the 3x3x3 candidate test on tiles held in LDS: the front-filtered stack is never stored; 0 = the plane-wise filter
 * writes it and the tiled detector reads it back.  Seeds are identical bit for bit. */
#define IA3_TUNE_SEED_FUSED 15
/* IA3_TUNE_SEED_SKIP: 1 = the fused detector of IA3_TUNE_SEED_FUSED leaves out the planes of a tile on which no
 * voxel can pass the candidate test: the column kernel reports the largest value of the short filter's axis-0 result per
 * plane, row and 32 columns, and a certified bound of max_im made from it (csrc/ia3_seedskip.h) is set against the
 * threshold and the lower bound of min_im; 2 (default) = and, with a dynamic threshold, the first-stage candidate list is
 * made at the first (highest) level instead of the lowest, with the seed stage started over at the lowest level when
 * level 0 yields fewer than min_dynamic_seeds seeds; 0 = every plane of every tile is filtered and tested, list at the
 * lowest level.  Seeds are identical bit for bit. */
#define IA3_TUNE_SEED_SKIP 16
/* IA3_TUNE_COL_RTC: per calling thread.  1 (default) = a stack depth without a built-in column kernel has it compiled at
 * run time the first time it is met (see ia3_prepare_depth); 0 = on this thread such a depth takes the sliding-window
 * pass unless its kernels are already loaded: no call starts the compiler.  fit_spots_by_segmentation, which filters one
 * crop per cell, each of a depth of its own, sets it around its loop.  Results are identical bit for bit. */
#define IA3_TUNE_COL_RTC 17
/* IA3_TUNE_SEED_BGORDER: 1 (default) = the sparse background pass of the lazy seed detector evaluates min_im on the
 * candidate's own plane first (nine values) and decides from them where it can: rejected below the threshold, accepted
 * with an in-plane neighbour below the centre; only the other candidates get the planes z - 1 and z + 1 (csrc/ia3_bgtest.h
 * states why this is the reference's test for every input); 0 = the same kernels evaluate all 27 values for every
 * candidate.  Seeds are identical bit for bit. */
#define IA3_TUNE_SEED_BGORDER 18
/* IA3_TUNE_DIST_TILE: output tile of the median kernel of ia3_dist_summary_dev.  0 (default) = 2 x 2 entries per workgroup
 * (64 lanes per entry) while 4 x 4 tiles would be fewer than two per compute unit, 4 x 4 (sixteen lanes per entry)
 * otherwise; 2, 4 or 8 = that tile for every shape (8 x 8: four lanes per entry).  Results are identical bit for bit. */
#define IA3_TUNE_DIST_TILE 19
/* IA3_TUNE_FIT_PAIR: 1 (default) = the two fits of a seed that IA3_TUNE_FIT_FUSE hands to one wavefront run together:
 * the evaluations stay full-wave and one after the other, the trust-region algebra between two evaluations runs for
 * both fits at once, one fit per half-wave; 0 = the same driver is called twice, one fit each time.  Tables are
 * identical bit for bit. */
#define IA3_TUNE_FIT_PAIR 20
/* IA3_DEBUG_FIT_MAXFEV: PROFILING ONLY, changes results: > 0 caps the function evaluations of every fit (MINPACK's maxfev),
 * which splits the fit kernel's time into its fixed and its per-evaluation part; 0 (default) = the reference's limits. */
#define IA3_DEBUG_FIT_MAXFEV 100
/* IA3_DEBUG_FIT_WAITBOUND: TESTS ONLY: polls after which a refit that waits for the fits it depends on gives up and the
 * launch aborts with IA3_EHIP ("a dependency wait exceeded its bound"); <= 0 (default) = 2^22 polls (~28 s, never reached
 * by a live kernel).  A small value makes ordinary waits of a crowded field trip it, which is how the abort path is
 * exercised; the call fails, nothing else changes. */
#define IA3_DEBUG_FIT_WAITBOUND 101
int ia3_set_tuning(int key, int value);

/* ---- device-resident stacks ----------------------------------------------------------------- */
int ia3_stack_upload(const void* host, int dtype, int Z, int X, int Y, ia3_stack** out);
int ia3_stack_alloc(int dtype, int Z, int X, int Y, ia3_stack** out);
/* Raw uint16 movie file -> resident (frames, X, Y) stack: what DaxReader(dax).loadAll() followed by an upload does
 * (visual_tools.py:974-1083), read in pieces through pinned staging buffers so file read and PCIe copy overlap.
 * offset_bytes: start of the first frame; big_endian != 0 swaps bytes on the device. */
int ia3_stack_load_file(const char* path, long long offset_bytes, int frames, int X, int Y, int big_endian,
                        ia3_stack** out);
int ia3_stack_wrap(void* devptr, int dtype, int Z, int X, int Y, ia3_stack** out); /* borrow device memory */
/* io_tools/load.py:524-550 split_im_by_channels on a resident raw movie (frames, X, Y): frames start, start+step, .. */
int ia3_stack_deinterleave(const ia3_stack* raw, int start, int step, int Z, ia3_stack** out);
/* device buffers for run-constant data (correction profiles) */
int ia3_buffer_upload(const void* host, size_t bytes, void** devptr);
void ia3_buffer_free(void* devptr);
/* a buffer of the same kind with undefined contents (for results made on the device), and its copy to the host */
int ia3_buffer_alloc(size_t bytes, void** devptr);
int ia3_buffer_download(const void* devptr, size_t bytes, void* host);
int ia3_stack_download(const ia3_stack* s, void* host);
int ia3_stack_info(const ia3_stack* s, int* dtype, int* Z, int* X, int* Y, void** devptr);
void ia3_stack_free(ia3_stack* s);

/* ---- filters ---------------------------------------------------------------------------------
 * scipy.ndimage.gaussian_filter semantics: per axis 0,1,2 a 1-D correlation accumulated in
 * float64 in NI_Correlate1D's order, re-quantised to the stack dtype after every axis (float32
 * rounds, uint16 truncates).  `weights` (2*radius+1 doubles) may be NULL, then they are
 * computed from (sigma, truncate) as scipy does.
 * Replaces: scipy.ndimage.gaussian_filter as called at spot_tools/fitting.py:92,99 and
 * correction_tools/filter.py:16. */
int ia3_gaussian_filter(const void* im, int dtype, int Z, int X, int Y, double sigma, double truncate,
                        int mode, const double* weights, int radius, void* out);
int ia3_gaussian_filter_dev(const ia3_stack* im, double sigma, double truncate, int mode,
                            const double* weights, int radius, ia3_stack* out);

/* correction_tools/filter.py:14-19 gaussian_high_pass_filter(image, sigma=5, truncate=2):
 * out = image - lowpass(nearest); out[lowpass > image] = 0, in the stack dtype. */
int ia3_gaussian_highpass(const void* im, int dtype, int Z, int X, int Y, double sigma, double truncate,
                          const double* weights, int radius, void* out);
int ia3_gaussian_highpass_dev(const ia3_stack* im, double sigma, double truncate,
                              const double* weights, int radius, ia3_stack* out);

/* correction_tools/filter.py:22-42 Remove_Hot_Pixels (and its twin corrections.py:490-510):
 * z-vote of im > hot_th * mean(4 rolled neighbours) -> column replaced by its 4-neighbour mean. */
int ia3_remove_hot_pixels(const void* im, int dtype, int Z, int X, int Y, double hot_pix_th, double hot_th,
                          void* out, int* n_hot);

/* Pre-corrections of io_tools/load.py:337-384 (correct_fov_image), uint16 outputs with NumPy's cast rules.
 * corrections.py:479-487 Z_Shift_Correction: out = u16(f32(im) / median_z * median_all); medians_out (Z+1
 * floats, per-plane then whole-stack) may be NULL. */
int ia3_z_shift_correction(const void* im, int dtype, int Z, int X, int Y, void* out_u16, float* medians_out);
/* io_tools/load.py:373-384: out = u16(f32(im) / profile[None]); profile (X,Y), prof_dtype 1 = float32, 2 = float64 */
int ia3_illumination_correct(const void* im_u16, int Z, int X, int Y, const void* profile, int prof_dtype,
                             void* out_u16);
/* io_tools/load.py:348-370: outs[i] = u16(clip(sum_j ims[j] * profile[i,j])); profile (C,C,X,Y), C <= 8 */
int ia3_bleedthrough_correct(const void* const* ims_u16, int C, int Z, int X, int Y, const void* profile,
                             int prof_dtype, void* const* outs_u16);

/* ---- order statistics of a resident stack and illumination profiles ----------------------------------------------
 * Exact selection (a radix select over the order-preserving key of the values; NaNs order last, as np.sort puts them).
 * ia3_stack_order_stats_dev: out[i] (host, n values of the stack dtype) = np.sort(stack, axis=None)[ranks[i]];
 * IA3_EINVAL for a rank outside [0, Z*X*Y) or n > 16. */
int ia3_stack_order_stats_dev(const ia3_stack* s, const long long* ranks, int n, void* out);
/* scipy.stats.scoreatpercentile(stack, per) as called at spot_tools/fitting.py:76 and
 * correction_tools/illumination.py:186-187: idx = per / 100. * (n - 1), the order statistic idx when that is a whole
 * number, else the two around it weighted in float64, (s[i] * w0 + s[i + 1] * w1) / (w0 + w1).  n <= 8 percentiles per
 * call, each in [0, 100] (else IA3_EINVAL); out: n doubles on the host. */
int ia3_stack_percentiles_dev(const ia3_stack* s, const double* pers, int n, double* out);
/* out_dev (X*Y doubles, device) = np.sum(float64(stack), axis=0), planes added in z order; clip != 0: every voxel is
 * first clamped to [lo, hi] as np.clip does (correction_tools/illumination.py:183-189). */
int ia3_clip_sum_z_dev(const ia3_stack* s, int clip, double lo, double hi, double* out_dev);
/* scipy.ndimage.gaussian_filter(float64 (X, Y) image, sigma, truncate=truncate, mode) in float64, bit for bit: axis 0
 * then axis 1, NI_Correlate1D's summation order.  `weights` (2 * radius + 1 doubles) are the taps SciPy would use, made
 * by NumPy on the caller's side (_lib.gaussian_taps) and used verbatim; NULL: they are made here from (sigma, truncate)
 * with libm's exp, which differs from NumPy's in the last bit for some arguments, so only explicit taps promise
 * bit-equal results.  mode reflect or nearest; radius up to 1024, larger ones IA3_EUNSUPPORTED.  out may be the input. */
int ia3_gaussian_filter2d_f64_dev(const double* in_dev, int X, int Y, double sigma, double truncate, int mode,
                                  const double* weights, int radius, double* out_dev);
int ia3_gaussian_filter2d_f64(const double* in, int X, int Y, double sigma, double truncate, int mode,
                              const double* weights, int radius, double* out);
/* correction_tools/illumination.py:181-190 for one channel stack (uint16 or float32): with remove_cap the limits are
 * the percentiles min(per_a, per_b) and max(per_a, per_b) of the stack; out_host (X*Y doubles) =
 * gaussian_filter(sum_z clip(float64(im), limits), sigma), taps as above (truncate 4).  Runs on the calling thread's
 * stream and waits for it. */
int ia3_illumination_image_profile_dev(const ia3_stack* im, int remove_cap, double per_a, double per_b, double sigma,
                                       const double* weights, int radius, double* out_host);

/* ---- seeding: spot_tools/fitting.py:20-154 get_seeds ------------------------------------------ */
typedef struct ia3_seed_params {
  double th_seed;               /* threshold on max_im - min_im */
  double gfilt_size;            /* 0.75 ; 0 = no front filter */
  double background_gfilt_size; /* 7.5  ; 0 = no background filter */
  int filt_size;                /* 3 */
  int min_edge_distance;        /* 2 */
  int use_dynamic_th;           /* 1 */
  int dynamic_niters;           /* 10 */
  int min_dynamic_seeds;        /* 1 */
  int remove_hot_pixel;         /* 1 */
  int hot_pixel_th;             /* 3 */
  int max_num_seeds;            /* <=0: unlimited */
  int th_compare_f32;           /* 1: each threshold level is rounded to float32 before the compare
                                   (NumPy>=2 weak-scalar rule for a Python-float th_seed, which is
                                   what fit_fov_image's float(th_seed) produces); 0: float64 compare
                                   (np.float64 th_seed, e.g. the percentile path) */
  const double* w_front; int r_front; /* optional explicit taps (NULL: from sigma, truncate 4) */
  const double* w_back;  int r_back;
} ia3_seed_params;

/* out_zxyh: capacity x 4 doubles [z,x,y,h], brightest first. */
int ia3_dog_seed(const void* im, int dtype, int Z, int X, int Y, const ia3_seed_params* p,
                 double* out_zxyh, int capacity, int* n_out, double* th_used);
int ia3_dog_seed_dev(const ia3_stack* im, const ia3_seed_params* p,
                     double* out_zxyh, int capacity, int* n_out, double* th_used);

/* The two filtered stacks get_seeds compares (spot_tools/fitting.py:83-96), as the seed detector computes them: `front`
 * = scipy.ndimage.gaussian_filter(im, sigma_front) complete, `back_axis0` = the FIRST pass of
 * gaussian_filter(im, sigma_back), i.e. scipy.ndimage.gaussian_filter1d(im, sigma_back, axis=0) — the detector runs the
 * other two passes of the background filter only around candidate maxima.  Both 'reflect', truncate 4, bit-identical
 * to SciPy.  On stacks of 30 / 40 / 50 planes with the default sigmas (0.75, 7.5) the two axis-0 passes share one
 * launch; every other case runs the separate filters.  Outputs must not alias the input or each other. */
int ia3_dog_filters_dev(const ia3_stack* im, double sigma_front, double sigma_back, ia3_stack* front, ia3_stack* back_axis0);

/* ---- chromatic-aberration profile generation (correction_tools/chromatic.py:119-412) --------------------------------
 * io_tools/crop.py:107-152 crop_neighboring_area(im, centre, crop, 'nearest') for n centres per resident stack, bit for
 * bit: rough crop, map_coordinates(order 3) on it, output of the stack's dtype.  a, b: stacks of equal shape and dtype (b
 * may be NULL: boxes of a alone); centers_a / centers_b: n x 3 float64 (z, x, y); crop[3]: box size per axis, 1..15
 * (larger: IA3_EUNSUPPORTED); crops_*_host: n x crop[0] x crop[1] x crop[2] of the stack dtype.  slope / intercept / rsq
 * (n doubles each, uint16 stacks only, else IA3_EUNSUPPORTED): the least-squares line box_b = slope * box_a + intercept
 * and its coefficient of determination (chromatic.py:387-390) from exact integer sums; constant box_a: slope 0,
 * intercept mean(box_b), rsq 0; constant box_b: rsq 1.  Every output pointer may be NULL.  A centre whose rough crop
 * does not meet the image is IA3_EINVAL. */
int ia3_crop_pairs_dev(const ia3_stack* a, const ia3_stack* b, const double* centers_a, const double* centers_b, int n,
                       const int* crop, void* crops_a_host, void* crops_b_host, double* slope, double* intercept,
                       double* rsq);
/* chromatic.py:282-289: *devptr = new buffer (free with ia3_buffer_free) holding the (3, Z, X, Y) field
 * out[a, z, x, y] = sum_k C_a[k] * m_k(z - ref_center[0], x - ref_center[1], y - ref_center[2]), m = the columns of
 * generate_polynomial_data(., orders[a]), summed left to right in float64 and stored as out_dtype (1 = float32,
 * 2 = float64: what ia3_warp3d_dev takes).  consts: the constants of axis 0, 1, 2 one after the other, n_cols[a] of
 * them (1, 4, 10, 20 for orders 0..3; higher orders: IA3_EUNSUPPORTED). */
int ia3_poly_field_dev(const double* consts, const int* n_cols, const int* orders, const double* ref_center, int Z, int X,
                       int Y, int out_dtype, void** devptr);

/* ---- bleedthrough profile generation (correction_tools/bleedthrough.py:451-486) -------------------------------------
 * consts: C*C blocks of n_cols doubles, block [tar*C + ref] = the polynomial of the slope profile from channel ref into
 * channel tar (columns of generate_polynomial_data(., order), 1/4/10/20 for order 0..3); present[tar*C + ref] == 0: the
 * zero profile (interploate_... returned np.zeros: not enough spots); diagonal blocks are ignored, the diagonal is 1.
 * M[tar, ref](z, x, y) = sum_k c_k m_k(z - rc0, x - rc1, y - rc2), summed left to right in float64.  mean_z != 0
 * (generate_2d): M is summed over z = 0..Z-1 in that order and divided by Z (what ndarray.mean(2) does), output
 * (C, C, X, Y); else output (C, C, Z, X, Y).  invert != 0: every C x C matrix is replaced by its inverse
 * (np.linalg.inv: elimination with partial pivoting); *n_singular = matrices with a zero pivot (their entries are NaN).
 * out_dtype 1 float32, 2 float64.  C 2..4, order 0..3, else IA3_EUNSUPPORTED.  *devptr: new buffer of the ia3_buffer_*
 * family. */
int ia3_bleedthrough_profile_dev(const double* consts, const unsigned char* present, int C, int order,
                                 const double* ref_center, int Z, int X, int Y, int mean_z, int invert,
                                 int out_dtype, void** devptr, long long* n_singular);

/* ---- the pre-correction chain of io_tools/load.py:323-384 on stacks that stay resident ---------------------------
 * ia3_remove_hot_pixels_dev works in place; float_arith != 0 on a uint16 stack = the chain's
 * corrections.Remove_Hot_Pixels(im.astype(np.float32), dtype=np.uint16) (float32 votes and means, one truncation at
 * the end).  Profiles are device buffers from ia3_buffer_upload; prof_dtype 1 = float32, 2 = float64.  Outputs of the
 * bleedthrough mix must not alias its inputs; the other two may run in place. */
int ia3_remove_hot_pixels_dev(ia3_stack* im, double hot_pix_th, double hot_th, int float_arith, int* n_hot);
int ia3_z_shift_correction_dev(const ia3_stack* im, ia3_stack* out_u16);
int ia3_illumination_correct_dev(const ia3_stack* im_u16, const void* profile_dev, int prof_dtype, ia3_stack* out_u16);
int ia3_bleedthrough_correct_dev(ia3_stack* const* ims_u16, int C, const void* profile_dev, int prof_dtype,
                                 ia3_stack* const* outs_u16);
/* the step-API twins in classes/preprocess.py (DaxProcesser._corr_illumination :605-680, ._corr_bleedthrough :464-541):
 * same quotient / mix (the mix accumulated in float64), then `(im - min) / (max - min) * 65535 + 0` when rescale != 0,
 * clip to [0, 65535], truncation */
int ia3_illumination_rescale_dev(const ia3_stack* im_u16, const void* profile_dev, int prof_dtype, int rescale,
                                 ia3_stack* out_u16);
int ia3_bleedthrough_rescale_dev(ia3_stack* const* ims_u16, int C, const void* profile_dev, int prof_dtype, int rescale,
                                 ia3_stack* const* outs_u16);

/* ---- background level: io_tools/load.py:642-687 find_image_background -----------------------------------
 * counts = np.histogram(im, bins=edges); highest strict local maximum of the counts (scipy.signal.find_peaks,
 * height halved from size/50 at most max_iter times); background = centre of that bin; np.nanmedian(im) when no
 * bin qualifies.  edges: the reference's np.arange(iinfo(dtype).min, iinfo(dtype).max, bin_size) as float64
 * (n_edges <= 16001). */
int ia3_find_background(const void* im, int dtype, int Z, int X, int Y, const double* edges, int n_edges,
                        int max_iter, double* background);
int ia3_find_background_dev(const ia3_stack* im, const double* edges, int n_edges, int max_iter, double* background);
/* spot_tools/fitting.py:246-258 (normalize_local=True): the same statistic over
 * io_tools/crop.py:59-88 generate_neighboring_crop(center, crop_size) for each of n centres (n x 3 float32, the
 * fitted [z,x,y] columns of the spot table), one block per spot. */
int ia3_local_background_dev(const ia3_stack* im, const float* centers_zxy, int n, int crop_size,
                             const double* edges, int n_edges, int max_iter, double* backgrounds);

/* ---- legacy per-cell seeding: visual_tools.py:1775-1870 get_seed_in_distance (+ :348-381 get_seed_points_base),
 * the seeder of classes/__init__.py:57-88 `_fit_single_image`.  Crop of +-seed_radius (x, y) / +-seed_radius/2 (z)
 * around `center` (NULL: whole image), scipy-default Gaussian filters (reflect, truncate 4), int64-truncated
 * rank-filter tests, strict '>' threshold lowered over np.linspace(1, 1/dynamic_iters, dynamic_iters) until enough
 * seeds lie within seed_radius, brightest num_seeds first.  th_seed is the resolved threshold (the shim evaluates
 * seed_by_per).  out_zxyh: capacity x 4 int64 [z, x, y, h]. */
typedef struct ia3_legacy_seed_params {
  int num_seeds;                 /* 0 = keep all */
  double seed_radius;            /* 30 */
  double gfilt_size;             /* 0.75 */
  double background_gfilt_size;  /* 10 */
  int filt_size;                 /* 3 */
  double th_seed;                /* 300 */
  int dynamic;                   /* 1 */
  int dynamic_iters;             /* 10 */
  int min_dynamic_seeds;         /* 2 */
  int hot_pix_th;                /* 4 */
} ia3_legacy_seed_params;
int ia3_seed_in_distance(const void* im, int dtype, int Z, int X, int Y, const double* center,
                         const ia3_legacy_seed_params* p, int64_t* out_zxyh, int capacity, int* n_out);

/* ---- fitting: External/Fitting_v4.py:559-683 iter_fit_seed_points (+ GaussianFit :165-396) ---- */
typedef struct ia3_fit_params {
  int radius_fit;            /* 5 */
  double min_delta_center;   /* 1.0  (firstfit) */
  double max_delta_center;   /* 2.5  (repeatfit) */
  int n_max_iter;            /* 10; the sweeps run are max(n_max_iter, 0) + 1 at most, as in the reference */
  double max_dist_th;        /* 0.1 */
  double min_w, max_w, init_w; /* 0.5, 4, 1.5; 0 < min_w < init_w < max_w, anything else is IA3_EINVAL */
  /* 0: External/Fitting_v4.py (production).  1: External/Fitting_v3.py:50-262,312-425, the fitter behind the
   * legacy classes/__init__.py:57-88 `_fit_single_image`: per-axis start widths init_w_zxy (the reference's
   * global _sigma_zxy = 1.35, 1.9, 1.9), its to_center (:81-87) and MINPACK's default maxfev. */
  int model_variant;
  double init_w_zxy[3];
} ia3_fit_params;

typedef struct ia3_fitter ia3_fitter;

/* centers_zxy: n x 3 doubles (the reference's `centers.T`).  The stack must stay alive until
 * ia3_fit_destroy. */
int ia3_fit_create(const ia3_stack* im, const double* centers_zxy, int n, const ia3_fit_params* p,
                   ia3_fitter** out);
int ia3_fit_first(ia3_fitter* f);                 /* .firstfit()  */
int ia3_fit_repeat(ia3_fitter* f, int* n_iter);   /* .repeatfit() */
int ia3_fit_run(ia3_fitter* f);                   /* .firstfit(); .repeatfit() in one persistent launch */
/* ps: n x 11 float32 rows [h,z,x,y,bk,sz,sx,sy,sin_t,sin_p,eps] (NaN rows for failed fits);
 * success: n bytes; nvox: n ints (voxels used by the last fit of each seed); any may be NULL. */
int ia3_fit_results(ia3_fitter* f, float* ps, uint8_t* success, int* nvox);
/* same, plus n_iter of the last repeatfit, with a single stream synchronisation */
int ia3_fit_results_ex(ia3_fitter* f, float* ps, uint8_t* success, int* nvox, int* n_iter);
/* nfev: n ints, model evaluations spent on each seed so far (first fit + sweeps); MINPACK stops a fit at maxfev */
int ia3_fit_nfev(ia3_fitter* f, int* nfev);
int ia3_fit_stats(ia3_fitter* f, int64_t* total_fits, int64_t* total_nfev);
/* the fitter's 32 device counters: [0] fits, [1] evaluations, [2] voxel evaluations; [8..31] shader cycles per phase in
 * a profiling build of the fit kernel (-DIA3_FIT_STAMPS, scripts/fit_stamps.sh), zero in the shipped library */
int ia3_fit_counters(ia3_fitter* f, uint64_t* out32);
void ia3_fit_destroy(ia3_fitter* f);

/* ---- views of a finished fit: what the reference's class leaves on the object besides the rows (gparms, ims_rec,
 * im_subtr, im_add; External/Fitting_v4.py:590-683).  The fit never materialises them; each call below renders one on
 * request from the fitter's per-seed records, with kernels of its own — ia3_fit_run and the per-FOV entries launch none of
 * this.  For a fitter of ONE field of view after ia3_fit_first / ia3_fit_run (several fields: IA3_EUNSUPPORTED, before the
 * first fit: IA3_EINVAL).  `which` selects the records: 0 = as ia3_fit_snapshot kept them (IA3_EINVAL without one), 1 = as
 * they are now.  nball below = voxels of the integer ball of radius_fit (offsets in [-r, r), 512 for radius 5). */
/* keeps a copy of the per-seed records as they are now (device to device, a block of its own from the scratch cache,
 * overwritten by the next call): called right after ia3_fit_first it is what im_subtr is made from later. */
int ia3_fit_snapshot(ia3_fitter* f);
/* gparms: per seed the voxels of its first fit — ball, image bounds, Voronoi cell with the fit's own tie decisions — packed
 * to the front in np.indices order of the ball.  counts: n ints; zxy: n x nball x 3 ints; vals: n x nball doubles (the image
 * values, exact); rows are filled up to counts[i].  The set depends on the seeds alone, hence no `which`. */
int ia3_fit_view_voxels(ia3_fitter* f, int* counts, int* zxy, double* vals);
/* ims_rec: per seed the model without background (GaussianFit.get_im) of its record over ball ∩ image, no Voronoi
 * restriction, packed the same way.  counts: n ints; has_rec: n bytes, 0 = no fit of this seed has succeeded (the
 * reference's scalar NaN; its row of recs is not written); recs: n x nball doubles; x11 (may be NULL): n x 11 doubles, the
 * record itself: the ten unconstrained parameters [bk, h, c0, c1, c2, w0, w1, w2, pp, tp] and the delta_center of that fit. */
int ia3_fit_view_recs(ia3_fitter* f, int which, int* counts, uint8_t* has_rec, double* recs, double* x11);
/* im_subtr (which = 0) / im_add (which = 1): Z x X x Y doubles on the host, per voxel ((im - rec_a) - rec_b) - ... over the
 * seeds a < b < ... with a reconstruction whose ball holds the voxel.  Bit-equal to the reference's im_subtr; its im_add is
 * updated in place and differs by the rounding order.  out == NULL: rendered on the device, waited for,
 * not copied (timing).  Same bits on every run.  Precondition: seeds whose balls share a voxel are within 2 radius_fit of
 * each other, which integer seed positions (ia3_dog_seed's) guarantee; the balls sit on the truncated positions, so
 * fractional seeds just beyond that distance would give a shared voxel two owners. */
int ia3_fit_view_residual(ia3_fitter* f, int which, double* out);
/* the same residual rounded once to float32 into a new resident stack (free it with ia3_stack_free): what a second
 * seeding pass reads; no float64 volume is made. */
int ia3_fit_view_residual_dev(ia3_fitter* f, int which, ia3_stack** out);
/* ia3_fit_create for several fields of view of the same shape and dtype (at most 64) in one fitter, seeds of field k =
 * n_seeds[k] x 3 doubles at centers_zxy[k]: neighbours and sweeps stay inside a field, the work list runs over all of them
 * (what ia3_fit_fovs makes per group).  Rows, success and nvox come back field after field. */
int ia3_fit_create_fovs(const ia3_stack* const* ims, const double* const* centers_zxy, const int* n_seeds, int n_fov,
                        const ia3_fit_params* p, ia3_fitter** out);

/* External/Fitting_v4.py:165-396 GaussianFit(im, X, center, ...).fit() for a batch of explicit voxel lists
 * (<= 512 voxels each): vals / coords_zxy concatenated, off[n_fits+1]; cfg4 = (delta_center, min_w, max_w,
 * init_w) per fit; kind = dtype class of the caller's values (0 float32, 1 integer, 2 float64), which selects
 * NumPy's arithmetic for the start point.  ps: n_fits x 11 (NaN row if < 10 voxels); xs: n_fits x 10
 * unconstrained solution (may be NULL); info: n_fits x 2 (success, nfev) (may be NULL). */
int ia3_gaussfit_voxels(const double* vals, const int* coords_zxy, const int* off, int n_fits,
                        const double* centers, const double* cfg4, const int* kind, float* ps, double* xs,
                        int* info);

/* one call: upload + firstfit + repeatfit */
int ia3_fit_seeds(const void* im, int dtype, int Z, int X, int Y, const double* centers_zxy, int n,
                  const ia3_fit_params* p, float* out_ps, uint8_t* success, int* n_iter);

/* seed + fit chained on a resident stack (the bench's hot path): fit_fov_image
 * (spot_tools/fitting.py:169-262) without the optional normalisation.  out_rows: capacity x 11
 * float32, NaN rows and out-of-image centres removed (fitting.py:232-237). */
int ia3_fit_fov_dev(const ia3_stack* im, const ia3_seed_params* sp, const ia3_fit_params* fp,
                    float* out_rows, int capacity, int* n_rows, int* n_seeds, int* n_iter);

/* fits run, model evaluations and voxel evaluations (sum over fits of evaluations x voxels) of the calling thread's
 * last ia3_fit_fov_dev: what the counted-flop rate of the fit kernel is computed from (bench.py). */
int ia3_fit_fov_stats(int64_t* fits, int64_t* nfev, int64_t* voxel_evals);
/* of the calling thread's last ia3_fit_fov_dev: shader cycles its fit waves spent waiting for the fits a refit depends on
 * (the reference's ordered sweeps, Fitting_v4.py:651-680), and the cycles those waves lived: the dependency-wait share */
int ia3_fit_fov_wait_share(int64_t* wait_cycles, int64_t* wave_cycles);

/* A batch of independent FOVs in one call: the per-image tasks the reference spreads over an mp.Pool
 * (classes/field_of_view.py:1129-1142, worker classes/batch_functions.py:60).  Each job is either a host stack
 * (uploaded here through pinned staging buffers while other jobs compute) or a resident one; `in_flight` jobs
 * (<= 0: 4, at most 64) are seeded side by side on library-owned threads and streams (at most 16) and fitted in groups
 * by one more.  Resident jobs may still be in production on the calling thread's stream: the batch waits for it.  Per job the outputs are those
 * of ia3_fit_fov_dev; the call returns the first failing job's code (every job's own code is in `rc`). */
typedef struct ia3_fov_job {
  const void* host;       /* (Z,X,Y) stack of `dtype` in host memory, or NULL */
  const ia3_stack* dev;   /* resident stack (used when not NULL) */
  float* rows;            /* capacity x 11 float32 */
  int capacity;
  int n_rows, n_seeds, n_iter, rc;          /* out */
  long long fits, nfev, voxel_evals;        /* out: see ia3_fit_fov_stats */
} ia3_fov_job;
int ia3_fit_fovs(ia3_fov_job* jobs, int n_jobs, int dtype, int Z, int X, int Y, const ia3_seed_params* sp,
                 const ia3_fit_params* fp, int in_flight);

/* ---- drift ------------------------------------------------------------------------------------
 * alignment_tools.py:286-328 fftalign_2d: (xt, yt) of the normalised full cross-correlation peak of two
 * 2-D float64 images inside a +-max_disp window around `center`. */
int ia3_fftalign_2d(const double* im1, int s1x, int s1y, const double* im2, int s2x, int s2y,
                    const double* center, double max_disp, int* out_xy);
/* alignment_tools.py:330-353 fft3d_from2d (gb <= 1): integer (tz, tx, ty) from z- then y-max-projections. */
int ia3_fft3d_from2d(const void* im1, const void* im2, int dtype, int Z, int X, int Y, double max_disp,
                     int* out_zxy);
int ia3_fft3d_from2d_dev(const ia3_stack* im1, const ia3_stack* im2, double max_disp, int* out_zxy);
/* Box-blur normalisation of a 2-D float32 image (sx x sy, host in, host out): cv2.blur(im, (gb, gb)) followed by
 * im / blurred (mode IA3_BLUR_DIVIDE, alignment_tools.py:278-283) or im - blurred (mode IA3_BLUR_SUBTRACT,
 * External/Fitting_v4.py:733-737).  Normalised gb x gb box, anchor gb / 2 in both axes (even gb is asymmetric), border
 * BORDER_REFLECT_101; each window summed in float64 (rows first), times the double 1 / gb^2, rounded to float32, then
 * the float32 divide / subtract.  Supported: 1 <= gb <= IA3_BLUR_MAX_GB; mode 1 needs gb >= 2 (gb = 1 subtracts the
 * image from itself); anything else is IA3_EINVAL.  OpenCV is not available to this project: the arithmetic follows its
 * published generic CV_32F path and is pinned against a NumPy restatement of the rules above only.  Exact in any
 * summation order for integer-valued images; for other float32 data OpenCV's running column sums may differ in the last
 * bit. */
#define IA3_BLUR_MAX_GB 32
#define IA3_BLUR_DIVIDE 0
#define IA3_BLUR_SUBTRACT 1
int ia3_blurnorm2d(const float* im, int sx, int sy, int gb, int mode, float* out);
/* fftalign_2d with the choice of offset convention and the correlation value.  convention IA3_OFFSET_ALIGNMENT_TOOLS:
 * -floor(cor.shape / 2) + [y, x] (what ia3_fftalign_2d returns); IA3_OFFSET_FITTING_V4: [y, x] - im2.shape + 1
 * (External/Fitting_v4.py:781) — the two agree only for images of one shape.  out_cor (may be NULL): the windowed peak
 * / prod(min(im1.shape, im2.shape)) (Fitting_v4.py:806). */
#define IA3_OFFSET_ALIGNMENT_TOOLS 0
#define IA3_OFFSET_FITTING_V4 1
int ia3_fftalign_2d_ex(const double* im1, int s1x, int s1y, const double* im2, int s2x, int s2y,
                       const double* center, double max_disp, int convention, int* out_xy, double* out_cor);
/* fft3d_from2d with the blur-normalised projections of gb > 1, all on the device: each max-projection is cast to float32,
 * normalised as by ia3_blurnorm2d (gb, mode) and correlated as by ia3_fftalign_2d_ex (convention).  mode 0 with gb <= 1
 * is the unblurred chain of ia3_fft3d_from2d; mode 1 (External/Fitting_v4.py:738-752) needs gb >= 2.  out_cor2 (may be
 * NULL): the correlation values of the xy and of the z stage. */
int ia3_fft3d_from2d_ex(const void* im1, const void* im2, int dtype, int Z, int X, int Y, int gb, int mode,
                        int convention, double max_disp, int* out_zxy, double* out_cor2);
int ia3_fft3d_from2d_dev_ex(const ia3_stack* im1, const ia3_stack* im2, int gb, int mode, int convention,
                            double max_disp, int* out_zxy, double* out_cor2);
/* skimage.registration.phase_cross_correlation(reference, moving, upsample_factor) as called at
 * correction_tools/alignment.py:491-494,631-632 and classes/preprocess.py:831-835 (published algorithm; pinned
 * against scikit-image 0.18.3 for normalization None, tests/golden/phase.npz).  normalization: 1 = "phase", 0 = None.  shift[3] = (dz, dx, dy) to apply to `moving`. */
int ia3_phase_xcorr3d(const void* ref, const void* mov, int dtype, int Z, int X, int Y, int upsample,
                      int normalization, double* shift, double* err, double* phasediff);
int ia3_phase_xcorr3d_dev(const ia3_stack* ref, const ia3_stack* mov, int upsample, int normalization,
                          double* shift, double* err, double* phasediff);
/* correction_tools/alignment.py:527-695 align_image, phase-correlation path (use_autocorr=True), on resident stacks: crop
 * after crop (crops: n_crops x 3 x 2 ints, [start, stop) per axis) skimage's phase_cross_correlation(ref crop, src crop,
 * upsample); as soon as >= min_good_drifts crops are in and >= min_good_drifts of them lie within drift_diff_th of their
 * mean, the mean of those is the drift (:664-674, flag 0); with no such agreement after the last crop, the mean of the
 * two closest drifts and the one nearest to both (:676-693, flag 1).  drifts_out (n_crops x 3, may be NULL) / n_used: the
 * per-crop drifts that were measured. */
int ia3_align_image_dev(const ia3_stack* src, const ia3_stack* ref, const int* crops, int n_crops, int upsample,
                        int normalization, int min_good_drifts, double drift_diff_th, double* drift, int* flag,
                        double* drifts_out, int* n_used);

/* Many images against ONE reference bead image (every movie of a run: classes/batch_functions.py:169-206): the half
 * spectra of the reference crops are computed once and kept on the device (105 MB per 50 x 512 x 512 crop), so a crop
 * costs two transforms instead of three.  ia3_align_image_ref = ia3_align_image_dev with such a reference; drifts are
 * identical.  A drift reference may be shared by several host threads; free it after their calls have returned. */
typedef struct ia3_drift_ref ia3_drift_ref;
int ia3_drift_ref_create(const ia3_stack* ref, const int* crops, int n_crops, ia3_drift_ref** out);
void ia3_drift_ref_free(ia3_drift_ref* r);
int ia3_align_image_ref(const ia3_stack* src, ia3_drift_ref* ref, int upsample, int normalization, int min_good_drifts,
                        double drift_diff_th, double* drift, int* flag, double* drifts_out, int* n_used);

/* ---- External/Fitting_v4.py fast path: box-normalised seeds and closed-form moment fits ---------------------------
 * normalzie_im (:94-98): new resident float32 stack = float32(im) minus its sz x sz box blur, plane by plane, with the
 * arithmetic of ia3_blurnorm2d (anchor sz / 2, BORDER_REFLECT_101, float64 window sums); 1 <= sz <= IA3_BLUR_MAX_GB,
 * larger boxes are IA3_EUNSUPPORTED. */
int ia3_fastfit_normalize_dev(const ia3_stack* im, int sz, ia3_stack** out);
/* get_seed_points_base_v2 (:100-126).  gfilt_size 0: the stack as it is, in its own dtype; otherwise its normalzie_im.
 * std_out = np.std of that stack, computed in float64 by fixed-order reductions and rounded to float32 for a float32
 * stack (NumPy sums in float32 there: the two agree to float32 rounding, not bit for bit).  Kept voxels: v > std * th_seed
 * (the product in float32 when th_f32 != 0 and the stack is float32: a Python number; else float64), v > 0 and v >= every
 * neighbour within filt_size / 2 on each axis, neighbours taken modulo the shape (filt_size / 2 <= 3).  zxyh: rows
 * [z, x, y, h], brightest first (equal heights: descending voxel order), at most max_num (< 0: all); *n_out their number;
 * IA3_ECAPACITY when it exceeds `capacity` rows. */
int ia3_fastfit_seeds_dev(const ia3_stack* im, int gfilt_size, int filt_size, double th_seed, int th_f32, int max_num,
                          double* zxyh, int capacity, int* n_out, double* std_out);
/* fast_fit_big_image (:496-558) with gfit_fast (:433-458) for every centre: out12 = n x 12 float64 rows [h, z, x, y, bk,
 * a, b, c, d, e, f, eps] (eps NaN; a row of NaN for a centre whose ball has no voxel in the image).  The ball: offsets
 * in [-radius_fit, radius_fit) with d^2 <= radius_fit^2 (radius_fit <= 5), at int(centre) + offset, clipped to the image;
 * avoid_neighbors: only the offsets nearer to this centre than to any other centre within 2 radius_fit (cdist's float64
 * arithmetic, ties to the lowest index); recenter: the ball is moved to its first maximum, the same offsets applied there.
 * uint16 stacks: the weights wrap as NumPy's uint16 subtraction does.  Optional (all three or none): vox_count[n] and the
 * voxel list each centre was fitted on, nball slots per centre (nball = number of ball offsets): vox_vals n x nball,
 * vox_zxy n x nball x 3. */
int ia3_fastfit_moments_dev(const ia3_stack* im, const double* centers_zxy, int n, int radius_fit, int avoid_neighbors,
                            int recenter, double bk_f, double* out12, int* vox_count, double* vox_vals, int* vox_zxy);
/* gfit_fast on one explicit voxel list (n <= 512): vals n float64 copies of the values, coords_zxy n x 3, kind the dtype
 * whose arithmetic the weights follow (0 float32, 1 uint16, 2 float64).  n = 0: twelve NaN. */
int ia3_fastfit_voxels(const double* vals, const int* coords_zxy, int n, int kind, double bk_f, double* out12);

/* ---- warp -------------------------------------------------------------------------------------
 * correction_tools/translate.py:5-31 warp_3d_image and its inlined twins (io_tools/load.py:438-453,
 * classes/preprocess.py:918-946): out = map_coordinates(im, grid (+ field) - drift, order, mode, cval).
 * orders 0 (nearest sample) and 1 with mode constant|nearest; order 3 (B-spline prefilter) with mode nearest (the production twins: padded by
 * 12, tuned kernels) or constant (warp_3d_image's default border mode: no padding, mirror-boundary prefilter, cval outside,
 * plain kernels; every axis >= 2 samples).
 * field: NULL or a (3,Z,X,Y) displacement field, field_dtype 1 = float32, 2 = float64; add 16 to form the
 * coordinates as (grid - drift) + field, the order of classes/preprocess.py:923-935 (DaxProcesser._warp_image),
 * instead of (grid + field) - drift. */
int ia3_warp3d(const void* im, int dtype, int Z, int X, int Y, const double* drift, const void* field,
               int field_dtype, int order, int mode, double cval, void* out);
int ia3_warp3d_dev(const ia3_stack* im, const double* drift, const void* field_dev, int field_dtype,
                   int order, int mode, double cval, ia3_stack* out);

/* new resident stack = s[z0:z1, x0:x1, y0:y1] (drift crops, correction_tools/alignment.py:617-622) */
int ia3_stack_crop(const ia3_stack* s, int z0, int z1, int x0, int x1, int y0, int y1, ia3_stack** out);

/* ---- segmentation label images (labels.hip) ------------------------------------------------------
 * A label (or mask) stack is an ordinary IA3_U16 stack; every result below is integer work, the reference's bit for bit
 * and the same on every run.
 * segmentation_tools/cell.py:598-611 segmentation_mask_2_bounding_box for every cell at once, in one pass over the
 * stack: out7 = (max_label + 1) rows [count, z0, z1, x0, x1, y0, y1] (host), row l the voxel count and the tight
 * [start, stop) bounds of label l, no margin; all zero for a label that does not occur and for row 0.  Labels above
 * max_label (1..65535) are passed over.  Stacks of up to 2^31 - 1 voxels (IA3_EUNSUPPORTED above). */
int ia3_label_boxes_dev(const ia3_stack* labels, int max_label, int* out7);
/* The cube of classes/partition_spots.py:212-236 find_coordinate_intensities around every row of centers_zxy (n x 3
 * float64, host): the centre rounded half to even (np.round(...).astype(np.int32)), the (2 radius + 1)^3 offsets in C
 * order of (dz, dx, dy), every index CLAMPED into the image (a cube that hangs over a face reads the face voxels several
 * times); radius 0..10.  Centres with NaN are outside the contract.  n = 0 launches nothing.
 * ia3_cube_labels_dev, target NULL: Spots_Partition.spots_to_labels (:113-140): out[i] = the most frequent label > 0 of
 * the cube, the smallest of equally frequent ones, -1 when the cube holds none.  target given (n ints): out[i] = 1 when
 * the cube holds target[i], else -1.
 * ia3_cube_max_dev: spots_to_DAPI (:143-157): out[i] = the largest value of the cube, in the stack dtype; NaN when a
 * float32 cube holds one.
 * ia3_cube_gather_dev: the (n, (2 radius + 1)^3) matrix itself, in the stack dtype. */
int ia3_cube_labels_dev(const ia3_stack* labels, const double* centers_zxy, int n, int radius, const int* target,
                        int* out);
int ia3_cube_max_dev(const ia3_stack* im, const double* centers_zxy, int n, int radius, void* out);
int ia3_cube_gather_dev(const ia3_stack* im, const double* centers_zxy, int n, int radius, void* out);

/* ---- candidate chromosomes: 3-D binary morphology and labelling (morph.hip) -----------------------
 * segmentation_tools/chromosome.py:264-361 find_candidate_chromosomes on a resident stack, and the operators it is made
 * of.  A mask is an IA3_U16 stack (0 / non-zero in, 0 / 1 out); inside the library it is one bit per voxel.  Order
 * statistics, comparisons, bit work and integer sums throughout: results equal NumPy / SciPy bit for bit and are the
 * same on every run.  Stacks of up to 2^31 - 1 voxels (IA3_EUNSUPPORTED above: int32 parents and labels).
 *
 * ia3_plane_medians_dev: out[z] = np.median(im[z]) as chromosome.py:296 divides by it, for all planes in one segmented
 * radix select: float64 (mean of the two middle values for an even count) for a uint16 stack; for a float32 stack the
 * float32 median (the two middle values added and halved in float32), widened.  NaN for a plane that holds one. */
int ia3_plane_medians_dev(const ia3_stack* im, double* out);
/* :293-311: mask_out = seed > scoreatpercentile(seed, binary_per_th) with the first and last ceil(filt_size / 2) planes,
 * rows and columns cleared, where seed = maximum_filter - minimum_filter (size filt_size = 1..5, window offsets
 * -(s / 2) .. s - 1 - s / 2, mode 'nearest') of im[z] / median(im[z]) in float64 (uint16 stack) or float32 (float32
 * stack).  *threshold = the percentile (float64, exact: a selection over the seed's own values); the compare is strict
 * and in float64.  IA3_EINVAL when a plane's median is 0 or not finite. */
int ia3_chrom_seed_mask_dev(const ia3_stack* im, int filt_size, double binary_per_th, ia3_stack* mask_out, double* threshold);
/* scipy.ndimage.binary_erosion / binary_dilation by skimage.morphology.ball(radius), radius 0..2 (ball(1) is the
 * 6-neighbour cross); border: what the outside of the volume counts as (0 or 1; SciPy's border_value).
 * IA3_MORPH_CLOSE = skimage.morphology.closing: dilation, then an erosion for which the outside counts as set (border
 * is not read).  out may be the input. */
#define IA3_MORPH_ERODE 0
#define IA3_MORPH_DILATE 1
#define IA3_MORPH_CLOSE 2
int ia3_binary_morph_dev(const ia3_stack* mask, int op, int radius, int border, ia3_stack* out);
/* scipy.ndimage.binary_fill_holes with the 6-neighbour cross (:319 with _morphology_size 1): every 6-connected component
 * of the background that touches no face of the volume is set.  out may be the input. */
int ia3_binary_fill_holes_dev(const ia3_stack* mask, ia3_stack* out);
/* scipy.ndimage.label, default structure (:325): labels_dev = device buffer of Z * X * Y int32 (ia3_buffer_alloc), 0 for
 * background and 1..n for the 6-connected components in raster order of their first voxel; *n_out = n.  labels16
 * (optional): the same as a uint16 stack; IA3_EUNSUPPORTED when n > 65535 (labels_dev and *n_out are complete then). */
int ia3_label_dev(const ia3_stack* mask, int* labels_dev, int* n_out, ia3_stack* labels16);
/* Labels are read from device memory: label_bits 32 = an int32 buffer as ia3_label_dev writes it, 16 = the voxels of a
 * uint16 stack (ia3_stack_info gives its pointer).  Labels above max_label count as background.
 * ia3_label_centers_dev: for l = 1..max_label, counts[l - 1] = the voxels of l and centers_zxy[3 (l - 1) ..] what
 * _calculate_binary_center (:4-10) gives for label == l: per axis the mean of the index over the voxels whose index on
 * that axis is > 0 (integer sum over count in float64; NaN when there is none).
 * ia3_remove_small_labels_dev: skimage.morphology.remove_small_objects on a labelled array (:337): labels with fewer
 * than min_size voxels become 0, the others keep their numbers; out_dev has the input's width and may be the input. */
int ia3_label_centers_dev(const void* labels_dev, int label_bits, int Z, int X, int Y, int max_label, double* centers_zxy,
                          long long* counts);
int ia3_remove_small_labels_dev(const void* labels_dev, int label_bits, int Z, int X, int Y, int max_label, long long min_size,
                                void* out_dev);
/* find_candidate_chromosomes (:264-361) in one call.  _adjust_layers, _random_walk_beta and _num_threads have no effect
 * there either: random_walker returns its labels when none of them is 0 (:326 leaves none).  morphology_size 1 only
 * (IA3_EUNSUPPORTED otherwise, and for more than 65535 components, where the reference wraps).  coords_zxy: capacity x 3
 * float64, the centres of the kept labels in ascending label order; *n_out their number (IA3_ECAPACITY with *n_out set
 * when capacity is too small; capacity 0 asks for the number).  kept_labels (optional): the uint16 label stack of :337. */
typedef struct ia3_chrom_params {
  int filt_size;            /* _filt_size */
  int morphology_size;      /* _morphology_size */
  int min_label_size;       /* _min_label_size */
  double binary_per_th;     /* _binary_per_th */
} ia3_chrom_params;
int ia3_find_candidate_chromosomes_dev(const ia3_stack* im, const ia3_chrom_params* p, double* coords_zxy, int capacity,
                                       int* n_out, double* threshold, ia3_stack* kept_labels);

/* ---- the chromosome image (chromim.hip) ----------------------------------------------------------------
 * classes/field_of_view.py:1821-1917 Field_of_View._generate_chrom_im_from_data: the float64 sum of every processed
 * round of a field of view, and find_candidate_chromosomes on it in the reference's float64 arithmetic.
 * An ia3_chrom_image is a float64 (Z,X,Y) volume in device memory; create gives zeros (np.zeros(single_im_size)),
 * upload / download copy the whole volume from / to Z * X * Y host doubles. */
typedef struct ia3_chrom_image ia3_chrom_image;
int ia3_chrom_image_create(int Z, int X, int Y, ia3_chrom_image** out);
void ia3_chrom_image_free(ia3_chrom_image* h);
int ia3_chrom_image_upload(ia3_chrom_image* h, const double* host);
int ia3_chrom_image_download(const ia3_chrom_image* h, double* host);
/* np.median of a whole resident stack, widened to float64: the middle order statistic, or for an even count the mean of
 * the two middle ones (uint16: in float64; float32: added and halved in float32).  NaN when the stack holds one. */
int ia3_stack_median_dev(const ia3_stack* s, double* out);
/* :1869-1891 (_fast): h += every one of the n resident uint16 stacks ims[k] of h's shape.  flags[k] == 2 (a warped image):
 * the image as it is.  Otherwise with d = shifts + 3 k (the rounded drift, z x y) and bg = np.median(ims[k]):
 * h[j] += ims[k][j + d] where j + d lies inside the stack and bg elsewhere, which is what `h += bg; h[dst] += im[src] - bg`
 * leaves: every term and partial sum is a multiple of 0.5 far below 2^52, so the sum is exact in any order.  The medians
 * are selected first, then the images are added in launches of up to 16, one read-modify-write of h per launch.
 * backgrounds_out (optional, n): the medians used, 0 for a warped image.  IA3_EUNSUPPORTED for a stack that is not uint16,
 * IA3_EINVAL for a shape other than h's and for |d| >= the axis length (NumPy cannot broadcast the two crops there). */
int ia3_chrom_image_add_dev(ia3_chrom_image* h, const ia3_stack* const* ims, const int* flags, const int* shifts, int n,
                            double* backgrounds_out);
/* ia3_find_candidate_chromosomes_dev on a chromosome image, in the float64 arithmetic NumPy uses for a float64 ndarray:
 * float64 plane medians (two middle values added and halved), IEEE float64 quotients, float64 seed.  Same outputs,
 * limits and errors. */
int ia3_find_candidate_chromosomes_f64_dev(const ia3_chrom_image* im, const ia3_chrom_params* p, double* coords_zxy,
                                           int capacity, int* n_out, double* threshold, ia3_stack* kept_labels);

/* ---- chromosome selection by candidate spots (select.hip) ------------------------------------------------
 * spot_tools/picking.py:767-794 assign_spots_to_chromosomes and the loop of segmentation_tools/chromosome.py:377-399
 * select_candidate_chromosomes.  Both take coordinates that are already scaled by distance_zxy (host NumPy), as n x 3 and
 * n_cand x 3 float64 host tables, n_cand >= 1 (at most 2^22).  The distance is scipy's cdist,
 * sqrt((dz*dz + dx*dx) + dy*dy) with every operation rounded to float64 on its own, and the owner of a spot is np.argmin of
 * its row: the first NaN if there is one, otherwise the first candidate whose ROOT is the smallest.
 * ia3_assign_nearest_dev: owner[i] (n ints) = that candidate for spot i. */
#define IA3_SELECT_THREADS 256   /* spots of one workgroup */
#define IA3_SELECT_TILE 256      /* candidates staged in LDS at a time */
#define IA3_SELECT_EMPTY 1       /* ia3_select_chromosomes_dev: every candidate was removed (outputs are complete) */
int ia3_assign_nearest_dev(const double* spots_zxy, int n, const double* cands_zxy, int n_cand, int* owner);
/* The selected spots of all n_rounds rounds packed in round order, round r = rows round_start[r] .. round_start[r + 1]
 * (round_start[0] = 0; an empty round repeats its start).  lost[c] = the rounds in which candidate c owns no spot; while the
 * largest double(lost) / n_rounds over the alive candidates is > loss_th, that candidate (the lowest index among equals) is
 * removed and only the spots it owned get a new owner among the alive ones.  removed[k] / removed_lost[k] (n_cand ints
 * each): index and lost of the k-th removed candidate, *n_removed their number; lost (n_cand ints): the final values (of a
 * removed candidate: undefined); owner (optional, n ints): the final owner of every spot; visits (optional): candidates
 * visited = n * n_cand + sum over the removals of (spots the candidate owned) * (candidates alive after it); times_ms
 * (optional, 3 doubles): host clock of the upload, the first pass and the removal loop, each ended by a synchronise
 * (the final downloads of lost and owner are in none of the three).
 * n_rounds = 0 removes nothing.  Returns IA3_SELECT_EMPTY when the last candidate was removed.  The host reads one
 * 8-byte record per removal step (four steps are queued per look); nothing that scales with n or n_cand moves between the first upload and the last download. */
int ia3_select_chromosomes_dev(const double* spots_zxy, const int* round_start, int n_rounds, const double* cands_zxy,
                               int n_cand, double loss_th, int* removed, int* removed_lost, int* n_removed, int* lost,
                               int* owner, long long* visits, double* times_ms);

/* ---- population spot picking (pick.hip) -------------------------------------------------------------------
 * spot_tools/picking.py:1567-2342: pick_spots_by_intensities, generate_reference_from_population (E-step),
 * pick_spots_by_scores (M-step), evaluate_differences and cum_val, on a population of P chromosomes x R regions that is
 * uploaded once and stays resident over the EM iterations.  Candidates: one packed n x 4 float64 table (h, z, x, y in nm);
 * region_start[P*R + 1]: CSR over (chromosome, region); row_1d[P*R]: 1 where the entry was given as ONE 1-D row (its norms
 * are BLAS ddot's sqrt(fma(dy,dy,fma(dx,dx,dz*dz))), those of a 2-D table sqrt((dz*dz+dx*dx)+dy*dy)); channel[R] in
 * 0..n_channels-1 (NULL and 0: no channels).  A key is a channel, or n_channels for 'all'; a kind is 0 centre distance,
 * 1 local-centre distance, 2 intensity.  Tables indexed [kind][key] are flat with IA3_PICK_MAX_CHANNELS + 1 keys per kind.
 * The local window of region j (:1689-1699) comes from the caller as CSR over reference indices in summation order:
 * win_idx[win_start[j] .. win_start[j + 1]), each in 0..R-1; np.nanmean adds the rows in that order.
 * Nothing that scales with P*R or n moves between create and the downloads: a step uploads the window table (R-sized),
 * optional centres (P x 3) and log tables (at most 2^16 values each), and reads back lengths or the 8-byte difference. */
#define IA3_PICK_MAX_CHANNELS 8
enum { IA3_PICK_ROWS_PICKS = 0, IA3_PICK_ROWS_PREV = 1, IA3_PICK_ROWS_REF = 2 };
enum { IA3_PICK_GET_PICKS = 0, IA3_PICK_GET_PREV = 1, IA3_PICK_GET_SEL_SCORES = 2, IA3_PICK_GET_PICK_INDEX = 3,
       IA3_PICK_GET_SCORES = 4, IA3_PICK_GET_MIDS = 5, IA3_PICK_GET_CAND_DISTS = 6, IA3_PICK_GET_REF_CT = 7,
       IA3_PICK_GET_REF_LOCAL = 8, IA3_PICK_GET_REF_INT = 9 };
typedef struct ia3_pick_population ia3_pick_population;
int ia3_pick_create(const double* cands, int n, const int* region_start, const unsigned char* row_1d, int P, int R,
                    const int* channel, int n_channels, ia3_pick_population** out);
void ia3_pick_free(ia3_pick_population* h);
/* :1723-1749: picks[p][r] = the first row of maximal h (np.argmax: the first NaN wins), a NaN row for an empty region */
int ia3_pick_by_intensity_dev(ia3_pick_population* h);
/* uploads a P*R x 4 table as the picks, the previous picks or the reference rows (IA3_PICK_ROWS_*) */
int ia3_pick_set_rows(ia3_pick_population* h, int which, const double* rows);
/* E-step (:1751-1876) of the picks against the reference rows (the picks themselves when ref_is_picks): per (chromosome,
 * region) the centre distance (centre: centers_zxy[P x 3], or NULL for the nanmean of the picks, per channel when split),
 * the local-centre distance and the intensity; their non-NaN values become the sorted reference arrays of 'all' and, when
 * split, of every channel.  lengths[kind][key]: the arrays' lengths, -1 for one that was not made. */
int ia3_pick_reference_dev(ia3_pick_population* h, const int* win_start, const int* win_idx, int split,
                           const double* centers_zxy, int ref_is_picks, int* lengths);
/* a sorted reference array given by the caller instead */
int ia3_pick_set_sorted(ia3_pick_population* h, int kind, int key, const double* values, int n);
/* M-step (:1906-2013): per candidate the distances, the three cum_val mids (order: centre, local, intensity; -1 for a
 * term whose weight is 0) and the score log_int + center_weight * log_ct + local_weight * log_lc (separate float64
 * operations, a term skipped when its weight is 0); per region the selected row (np.argmax: the first NaN, else the first
 * maximum), its score (np.nanmax) and its index in the region (-1: empty).  The picks become the previous picks and the
 * selection the picks.  logtabs[kind][key] (host, logsizes values): for every array a score reads, indexed by the heap
 * number of the search node a cum_val ends on (root 1, a true compare goes to 2 * node + 1), np.log(mid / n) for kind 2
 * and np.log(1 - mid / n) for kinds 0 and 1, mid = 0.5 where the node's mid is 0, evaluated by the host's NumPy.
 * A table is a function of its array's length alone: it is copied to the device only when that length (or logsizes) differs
 * from the one the resident table was made for.
 * IA3_EINVAL when an array a score reads is empty (the reference's IndexError).  dist_only: the distances alone. */
int ia3_pick_scores_dev(ia3_pick_population* h, const int* win_start, const int* win_idx, int split_int, int split_dist,
                        double center_weight, double local_weight, const double* centers_zxy, int ref_is_picks,
                        const double* const* logtabs, const int* logsizes, int dist_only);
/* :2280-2284: counts[0] = rows whose picks moved by less than 0.01, counts[1] = rows whose distance is not NaN */
int ia3_pick_difference_dev(ia3_pick_population* h, int* counts);
/* IA3_PICK_GET_*: picks / previous picks (P*R x 4 float64), selected scores (P*R float64), pick index (P*R int32), scores
 * (n float64), mids (n x 3 int32), candidate distances (n x 2 float64: centre, local), the E-step's values (P*R float64) */
int ia3_pick_download(ia3_pick_population* h, int what, void* out);
int ia3_pick_download_sorted(ia3_pick_population* h, int kind, int key, double* out);
/* :1879-1899 cum_val alone: mids[i] = the last mid of the search for targets[i] in sorted_vals[0..n), n >= 1 */
int ia3_pick_cum_vals_dev(const double* sorted_vals, int n, const double* targets, int m, int* mids);

/* ---- summaries of population distance maps (distsum.hip) ----------------------------------------------------
 * structure_tools/distance.py:12-67: per chromosome pair the stack of squareform(pdist(zxys)) / cdist(zxys1, zxys2)
 * matrices over all cells and homolog combinations, reduced along the stack by np.nanmedian, np.nanmean or contact_prob.
 * The stack is never made.  A population is the packed rows x 3 float64 (z, x, y) tables of M chromosome copies, copy m =
 * rows copy_start[m] .. copy_start[m + 1]; it is uploaded once (region-major per group of copies with equally many rows)
 * and stays resident.  A summary names N >= 1 pairs of copies whose tables have Ra and Rb rows.  The distance is scipy's,
 * sqrt(q) with q = (dz*dz + dx*dx) + dy*dy, every operation rounded to float64 on its own; same = 1: pair_a[n] ==
 * pair_b[n] and the diagonal is squareform's literal 0, also for a row of NaNs.
 *   IA3_DIST_NANMEDIAN  per entry the middle one of the sorted values that are not NaN, (lo + hi) / 2.0 of the two middle
 *                       ones for an even count, NaN for none: selected on q (sqrt is monotone), two roots per entry
 *   IA3_DIST_NANMEAN    the roots added in the order of n with NaN as 0 (pairwise, as NumPy, when Ra * Rb == 1), over the
 *                       count of values that are not NaN
 *   IA3_DIST_CONTACT    n_contact / n_finite in float64 (0 / 0: NaN), n_contact = values <= contact_th counted as
 *                       q <= q* (csrc/ia3_distsum.h: the largest double whose root is <= contact_th; no contact for a
 *                       negative or NaN threshold, every value that is not NaN for +inf), n_finite = finite values
 * out: Ra x Rb float64; n_finite / n_contact: optional Ra x Rb int32 (contact_th is read only for them and for
 * IA3_DIST_CONTACT).  Host pointers.  Device memory of a call beyond the resident tables: 2 N ints and 16 Ra Rb bytes,
 * whatever N * Ra * Rb is; nothing of that size is made, moved or downloaded.  IA3_EINVAL: N < 1, a copy index outside
 * 0..M-1, a pair whose tables do not have Ra / Rb rows, same with pair_a[n] != pair_b[n]. */
enum { IA3_DIST_NANMEDIAN = 0, IA3_DIST_NANMEAN = 1, IA3_DIST_CONTACT = 2 };
typedef struct ia3_dist_population ia3_dist_population;
int ia3_dist_create(const double* zxys, const int* copy_start, int M, ia3_dist_population** out);
void ia3_dist_free(ia3_dist_population* h);
int ia3_dist_summary_dev(ia3_dist_population* h, const int* pair_a, const int* pair_b, int N, int Ra, int Rb, int same,
                         int function, double contact_th, double* out, int* n_finite, int* n_contact);
/* distance.py:231-232 contact_prob of an (N, K) float64 stack the caller holds (host): `value <= contact_th` on the values
 * themselves over np.isfinite; prob: K float64, n_finite / n_contact: optional K int32 */
int ia3_dist_contact_stack_dev(const double* stack, long long N, long long K, double contact_th, double* prob, int* n_finite,
                               int* n_contact);

/* ---- A/B compartment densities of traced cells (density.hip) --------------------------------------------------
 * compartment_tools/density.py:4-102: for every locus of every cell, the sum over the A loci and over the B loci of the
 * cell's other chromosome copies (trans) and / or of its own copy (cis) of
 *   exp(t),  t = -0.5 * ((dz*dz / s2[0] + dx*dx / s2[1]) + dy*dy / s2[2]),  d = contributor - query,
 * every operation of t rounded to float64 on its own (csrc/ia3_density.h) and exp the device library's float64 exp.
 * A population is the packed n_points x 3 float64 (z, x, y) loci of n_cells cells, cell c = points cell_start[c] ..
 * cell_start[c + 1] (at most IA3_DENSITY_MAX_CELL of them); copy_of[p] numbers the point's (chromosome, homolog) within its
 * cell (0 .. IA3_DENSITY_MAX_CELL - 1) and locus_of[p] in 0 .. n_loci - 1 names its (chromosome, region).  It is uploaded
 * once and stays resident; a point with a coordinate that is not finite contributes to no sum.
 * A scoring call names, per locus id, how often it counts as A and as B: mult[2 * id] and mult[2 * id + 1].  A contributor
 * of another copy weighs use_trans ? mult : 0, one of the query's own copy use_cis && mult > 0 ? 1 : 0, and with exclude_self
 * the query itself 0.  sums[k * n_points + p] (k = 0: A, 1: B) is the weighted sum of point p, added as partial sums of at
 * most 64 consecutive contributors and then the partial sums in order (no atomics: the same bits on every run, whatever
 * other cells the population holds); NaN for a query with a NaN coordinate.  counts[k * n_points + p] is the sum of the
 * weights, the number of rows the reference would add.  Host pointers; per call 2 n_loci + 24 bytes go up and
 * 24 n_points come down.  IA3_EINVAL: a null pointer, n_cells < 1, n_loci < 1, a cell_start that does not begin at 0 or
 * falls, a cell above the cap, an id out of range, neither use_cis nor use_trans.  The handle is an
 * ia3_density_population of density.hip. */
#define IA3_DENSITY_MAX_CELL 65536
int ia3_density_create(const double* zxys, const int* cell_start, const int* copy_of, const int* locus_of, int n_cells,
                       int n_loci, void** out);
void ia3_density_free(void* h);
int ia3_density_scores_dev(void* h, const unsigned char* mult, const double* s2, int use_cis, int use_trans, int exclude_self,
                           double* sums, int* counts);

/* ---- density clouds of traced chromosomes (cloud.hip) ---------------------------------------------------------
 * visual_tools.py:68-72 gauss_ker, :87-116 add_source and the loop of structure_tools/chromosome.py:5-57
 * convert_chr2Zxys_2_Cloud over the loci of a homolog.  A source is eight float64: pos[3], h, sig[3], size_fold.  With
 *   s = int(max(sig) * size_fold),  pos_int = trunc(pos),  disp = -pos_int + pos,  pos_min = trunc(pos_int - (s + 1) / 2.)
 * it adds, to every voxel i of [in_im(pos_min), in_im(pos_min + s + 1)) (in_im: >= shape becomes shape - 1, < 0 becomes 0,
 * so the last plane of an axis is never written),
 *   h * exp(t),  t = -((u0*u0 + u1*u1) + u2*u2) / 2.,  u_k = ((a_k - disp[k]) - s / 2.) / (sig[k]*sig[k]),
 * where the kernel's coordinates (a_0, a_1, a_2) of voxel i are (i[1] - pos_min[1], i[2] - pos_min[2], i[0] - pos_min[0]):
 * np.swapaxes(np.indices(...), 0, 3) pairs array axis 0 with disp[2] and sig[2], axis 1 with entry 0 and axis 2 with entry 1.
 * Every operation of t is rounded to float64 on its own (csrc/ia3_cloud.h), t < -746 gives +0 and exp is the device
 * library's float64 exp.  The n_images images of a call have one shape d0 x d1 x d2; image i takes the sources
 * image_start[i] .. image_start[i + 1] of the table IN THAT ORDER.  mode IA3_CLOUD_F64: float64 images, acc = acc + h*exp(t)
 * (add_source); IA3_CLOUD_F32: float32 images, acc = float32(float64(acc) + h*exp(t)) after every source (what assigning
 * add_source's result into a float32 slice does, chromosome.py:35).  One launch for all images; a voxel's result does not
 * depend on the other images of the call.  `sources` and `image_start` are host pointers in both forms.
 *   ia3_cloud_render_dev   d_images is device memory (ia3_buffer_alloc) of n_images * d0 * d1 * d2 values of the mode's type,
 *                          zeroed first when zero_first is set, else added to; it has been written when the call returns.
 *   ia3_cloud_render       host images: `init` (the mode's type, or NULL for zeros) goes up and `out` comes down.
 *   ia3_cloud_gauss_ker    the bare (s + 1)^3 float64 kernel of gauss_ker(sig, s, disp), host pointers; disp is any three
 *                          values.  s is 0 .. IA3_CLOUD_MAX_KER_S.
 * IA3_EINVAL, before any launch and before the device is touched: a null pointer, a mode other than the two, n_images outside
 * 1 .. IA3_CLOUD_MAX_IMAGES, a dimension outside 1 .. IA3_CLOUD_MAX_DIM, an image_start that does not begin at 0 or falls,
 * a source whose pos, sig or size_fold is NaN or infinite or whose s is outside 0 .. IA3_CLOUD_MAX_S.  A zero sigma is taken:
 * IEEE division gives the reference's 0 or NaN.  A source whose box lies outside the image adds nothing. */
#define IA3_CLOUD_F64 0
#define IA3_CLOUD_F32 1
#define IA3_CLOUD_MAX_S 4096
#define IA3_CLOUD_MAX_KER_S 511
#define IA3_CLOUD_MAX_IMAGES 65535
#define IA3_CLOUD_MAX_DIM 4096
int ia3_cloud_render_dev(const double* sources, const int* image_start, int n_images, int d0, int d1, int d2, int mode,
                         int zero_first, void* d_images);
int ia3_cloud_render(const double* sources, const int* image_start, int n_images, int d0, int d1, int d2, int mode,
                     const void* init, void* out);
int ia3_cloud_gauss_ker(const double* sig, int s, const double* disp, double* out);

/* ---- domain distances of traced chromosomes: domain_tools/distance.py (csrc/domain.hip) ------------
 * ia3_domain_create uploads a population once: N copies x R loci of (z, x, y) float64 coordinates, NaN for a missing locus
 * (is_matrix 0), or ONE R x R float64 distance map (is_matrix 1, N must be 1); `norm` is NULL or one R x R float64
 * normalisation map shared by all copies (the caller has checked that it is symmetric with a zero diagonal).  A distance
 * d[r, c] is sqrt((dz*dz + dx*dx) + dy*dy) of loci r and c (scipy's pdist / cdist arithmetic) or entry [r, c] of the map,
 * divided by norm[r, c] where a call sets use_norm.  Host pointers in, host pointers out; each call waits once.
 *   ia3_domain_slide_dev     _sliding_window_dist (:19-67) of every copy for W window sizes (1 .. IA3_DOMAIN_MAX_WINDOW each,
 *                            W <= IA3_DOMAIN_MAX_WINDOWS): out is (N, W, R) float64.  For coordinates the map is
 *                            squareform(pdist(zxy)).  Equal to the reference in every bit; where it gives NaN, a NaN.
 *   ia3_domain_dists_dev     domain_distance (:69-158) for Q entries (copy, s1, e1, s2, e2) of int32: the two domains are the
 *                            loci [s1, e1) and [s2, e2).  metric IA3_DOMAIN_DIST_*; int_zero[q] is 1 where Python returns
 *                            the integer 0 (a set without a value that is not NaN, or max(_final_dist, 0) took the 0) and
 *                            out[q] is then 0.
 *   ia3_domain_contacts_dev  one block of _domain_contact_freq (:465-490) per entry: n_contact[q] (optional) entries of
 *                            d[s1:e1, s2:e2] are <= contact_th, freq[q] is that count over the block's size (0 / 0: NaN);
 *                            for coordinates d is squareform(pdist(zxy)), diagonal 0.  A NaN is never a contact.
 * IA3_EINVAL before any launch: a null pointer, Q < 1, an entry whose copy or bounds lie outside the population
 * (0 <= s <= e <= R), a metric outside its list, a window size < 1, use_norm without a map.  IA3_EUNSUPPORTED: R above
 * IA3_DOMAIN_MAX_R, a window size above IA3_DOMAIN_MAX_WINDOW, more than 2^31 - 1 windows in one call. */
#define IA3_DOMAIN_MAX_WINDOW 16
#define IA3_DOMAIN_MAX_WINDOWS 16
#define IA3_DOMAIN_MAX_R 16384
#define IA3_DOMAIN_WINDOW_MEDIAN 0
#define IA3_DOMAIN_WINDOW_MEAN 1
#define IA3_DOMAIN_WINDOW_KS 2
#define IA3_DOMAIN_WINDOW_NORMED_INSULATION 3
#define IA3_DOMAIN_WINDOW_INSULATION 4
#define IA3_DOMAIN_DIST_MEDIAN 0
#define IA3_DOMAIN_DIST_ABSOLUTE_MEDIAN 1
#define IA3_DOMAIN_DIST_INSULATION 2
int ia3_domain_create(const double* data, int N, int R, int is_matrix, const double* norm, void** out);
void ia3_domain_free(void* population);
int ia3_domain_slide_dev(void* population, const int* window_sizes, int W, int metric, int use_norm, double* out);
int ia3_domain_dists_dev(void* population, const int* quads, int Q, int metric, int allow_minus, int use_norm, double* out,
                         int* int_zero);
int ia3_domain_contacts_dev(void* population, const int* quads, int Q, double contact_th, double* freq, int* n_contact);

/* ---- chromosomal spot scores: spot_tools/scoring.py (csrc/score.hip) ------------------------------
 * ia3_score_create uploads C traced chromosomes once, as CSR: chromosome c owns the candidate rows
 * cand_start[c] .. cand_start[c + 1] and the selected rows sel_start[c] .. sel_start[c + 1] (at least one of each).  A row
 * is (h, z, x, y) float64 with the coordinates in pixels, its region id an int64 that must lie in int32.  center: (C, 3)
 * chromosome centres in pixels, used where has_center[c] is non-zero (either may be null: no centre is given);
 * distance_zxy: the three pixel sizes.  ia3_score_replace_selected swaps the selected rows (the candidates stay).
 *   ia3_score_refs_dev   generate_ref_from_chromosome (:217-303) of every chromosome.  half = int((local_size - 1) / 2).
 *                        arrays (4, S): the centre, local and neighbour distances and the filtered intensities of the S
 *                        selected rows, chromosome by chromosome; with ignore_nan each chromosome's values are moved
 *                        to the front of its stretch without their NaNs (in row order) and a stretch left empty holds
 *                        the reference's fallback value.  counts (C, 4): the values of each stretch, -1 where the
 *                        one value is that fallback; scalars (C, 4): by
 *                        ref_metric IA3_SCORE_REF_* the nanmedian, the nanmean or the radius of gyration (not for _CDF;
 *                        the fourth is not set for _RG).
 *   ia3_score_scores_dev the four scores of every candidate up to the argument of np.log.  geom (5, N): centre, local,
 *                        forward, reverse and mean neighbour distance of the N candidates (step / invalid:
 *                        neighbor_step / invalid_dist of :180).  kind < 0: only those.  Otherwise kind is
 *                        IA3_SCORE_KIND_DIST_LINEAR or _DIST_CDF, the references are made from the selected rows by
 *                        ref_metric (IA3_SCORE_REF_CDF with the cdf kind) and val / cls (4, N) hold for the centre,
 *                        local, neighbour and intensity score a value and what is left to do with it: 0 it is the
 *                        score, 1 the score is np.log(value) * weight, 2 the score is -inf; 4 is added where the
 *                        distance or intensity was NaN.  ref_counts (C, 4): the values of each reference without NaNs.
 *   ia3_score_values_dev the same for n values x against one reference given by the caller: kind IA3_SCORE_KIND_* (also
 *                        _INT_LINEAR, _INT_CDF and _CUM_PROB, the plain _cum_prob of :81-107); ref_array (n_ref values,
 *                        NaNs dropped, sorted on the device) for the cdf kinds, ref_scalar for the linear ones.
 *   ia3_score_neighbor_lists_dev   neighboring_distances with use_median=False: every distance between a candidate and
 *                        the candidates of region id + step (fwd) and id - step (rev) where id + step is a region,
 *                        else `invalid` once in both; off_fwd / off_rev (N + 1): where each candidate's values start.
 * IA3_EINVAL before any launch for null pointers, an empty population or chromosome, row offsets that do not ascend, an
 * id outside int32, more than IA3_SCORE_MAX_PER_REGION rows of one region id in a chromosome and a half window above
 * (IA3_SCORE_MAX_LOCAL - 1) / 2. */
#define IA3_SCORE_MAX_PER_REGION 64
#define IA3_SCORE_MAX_LOCAL 33
#define IA3_SCORE_KIND_DIST_LINEAR 0
#define IA3_SCORE_KIND_DIST_CDF 1
#define IA3_SCORE_KIND_INT_LINEAR 2
#define IA3_SCORE_KIND_INT_CDF 3
#define IA3_SCORE_KIND_CUM_PROB 4
#define IA3_SCORE_REF_MEDIAN 0
#define IA3_SCORE_REF_MEAN 1
#define IA3_SCORE_REF_RG 2
#define IA3_SCORE_REF_CDF 3
int ia3_score_create(const double* cand, const long long* cand_id, const int* cand_start, const double* sel,
                     const long long* sel_id, const int* sel_start, const double* center, const int* has_center, int C,
                     const double* distance_zxy, void** out);
int ia3_score_replace_selected(void* population, const double* sel, const long long* sel_id, const int* sel_start);
void ia3_score_free(void* population);
int ia3_score_refs_dev(void* population, int ref_metric, int half, double intensity_th, int ignore_nan, double* arrays,
                       int* counts, double* scalars);
int ia3_score_scores_dev(void* population, int kind, int ref_metric, int half, long long step, double invalid,
                         double intensity_th, int ignore_nan, const double* weights, double limit_lo, double limit_hi,
                         double* geom, double* val, unsigned char* cls, int* ref_counts);
int ia3_score_values_dev(const double* ref_array, int n_ref, double ref_scalar, const double* x, int n, int kind,
                         double weight, double limit_lo, double limit_hi, double* val, unsigned char* cls, int* ref_count);
int ia3_score_neighbor_lists_dev(void* population, long long step, double invalid, const int* off_fwd, const int* off_rev,
                                 double* fwd, double* rev);

/* ---- per-cell spot pickers: spot_tools/picking.py :662-1563 (csrc/cellpick.hip) ------------------
 * ia3_cellpick_create uploads the candidates of n_cells cells once, as CSR over cell x region x chromosome: cell k owns
 * the regions [region_start[k], region_start[k + 1]) of G in all, has n_chrom[k] chromosomes (at most
 * IA3_CELLPICK_MAX_CHROM) and, where has_coords[k] is non-zero, their coordinates coords[(k * IA3_CELLPICK_MAX_CHROM + c)
 * * 3 ..] in pixels; chromosome c of region g owns the rows [cand_start[g * IA3_CELLPICK_MAX_CHROM + c], cand_start[.. + 1])
 * of `rows` ((n, 4): h, z, x, y in pixels); row_nan[i] is non-zero where candidate i holds a NaN in any column of the
 * caller's table.  cap_start (G + 1): where each region's merged rows start; region g must get room for its candidates
 * plus 2 * n_chrom rows.
 *   ia3_cellpick_merge_dev   merge_spot_list (:662-765) of every region, the merged rows kept on the device.  has_th == 0:
 *                            intensity_th None.  Out: count / valid (G) merged rows and those of them without a NaN;
 *                            src (cap_start[G]): per merged row its candidate, or -(1 + chromosome) for a placeholder.
 *   ia3_cellpick_naive_dev   the selections of naive_pick_spots_for_chromosomes (:854-888): mode _NAIVE_OWN picks per
 *                            chromosome among its own candidates (pick: the candidate or -1), _NAIVE_MERGED among the merged
 *                            rows nearest to its coordinate (pick: the merged row of the region, sub: its index among the
 *                            chromosome's rows).  pick / sub: (G, IA3_CELLPICK_MAX_CHROM).
 *   ia3_cellpick_plan        the regions each cell's forward pass walks, in its order: cell k walks
 *                            vreg[vstart[k] .. vstart[k + 1]); vgap: the id of each minus the id of the one before (0 for
 *                            the first).  Every region named must have 1 to IA3_CELLPICK_MAX_SPOTS merged rows.
 *   ia3_cellpick_forward_dev the forward pass (:1093-1155) of the n_active cells `cells` (ascending).  scores
 *                            (max n_chrom, cap_start[G]): per chromosome the score of every merged row; kind:
 *                            IA3_SCORE_KIND_DIST_LINEAR with ref_scalar (n_cells, IA3_CELLPICK_MAX_CHROM), or _DIST_CDF with
 *                            per (cell, chromosome) the sorted reference values [ref_start[j], ref_start[j + 1]) of `sorted`
 *                            and the ref_start[j + 1] - ref_start[j] + 1 scores at table[ref_start[j] + j ..].  Out: dy, the
 *                            dynamic scores, and ptr, the chosen row of the region before (255 where none), laid out as
 *                            scores; err (n_cells): 0, 1 where no tuple of distinct rows exists, 2 where no sum is a number,
 *                            3 where a spot would walk more than IA3_CELLPICK_MAX_TUPLES index tuples (every score of a
 *                            chromosome infinite, so all its rows are allowed): that spot is not picked.
 *                            The planes: scores, dy and ptr hold one plane of cap_start[G] values per chromosome up to the
 *                            largest n_chrom of the population, not IA3_CELLPICK_MAX_CHROM.  _NAIVE_MERGED picks nothing
 *                            for a cell without coordinates.
 * IA3_EINVAL before any launch for null pointers, offsets that do not ascend, more chromosomes than built, and regions,
 * cells or reference ranges out of bounds. */
#define IA3_CELLPICK_MAX_CHROM 6
#define IA3_CELLPICK_MAX_SPOTS 64
#define IA3_CELLPICK_MAX_TUPLES 4194304
#define IA3_CELLPICK_NAIVE_OWN 0
#define IA3_CELLPICK_NAIVE_MERGED 1
int ia3_cellpick_create(const double* rows, const unsigned char* row_nan, const int* cand_start, const int* region_start,
                        const int* n_chrom, const double* coords, const int* has_coords, const int* cap_start, int n_cells,
                        int G, const double* distance_zxy, void** out);
void ia3_cellpick_free(void* population);
int ia3_cellpick_merge_dev(void* population, int has_th, double intensity_th, int hard, double dist_th, int* count, int* valid,
                           int* src);
int ia3_cellpick_naive_dev(void* population, int mode, int* pick, int* sub);
int ia3_cellpick_plan(void* population, const int* vstart, const int* vreg, const long long* vgap);
int ia3_cellpick_forward_dev(void* population, const int* cells, int n_active, const double* scores, int kind,
                             const double* ref_scalar, const int* ref_start, const double* sorted, const double* table,
                             double weight, double limit_hi, double nan_mask, int share, double* dy, unsigned char* ptr, int* err);

/* ---- whole round-folder movies: the per-image task of classes/batch_functions.py:60-302 batch_process_image_to_spots
 * (fanned out over an mp.Pool by classes/field_of_view.py:1027-1142), as ONE pipelined call over many movies -------------
 * Per movie: raw (frames, X, Y) uint16 movie from host memory or a .dax file -> split_im_by_channels
 * (io_tools/load.py:524-550) -> hot pixels, z shift, bleedthrough, illumination (:323-384) -> bead drift against the
 * resident reference bead stack (align_image, phase correlation) -> cubic warp with drift + dense chromatic field
 * (:424-453) -> (Gaussian high-pass :489-498) -> get_seeds + firstfit + repeatfit + row filters of every selected channel
 * (spot_tools/fitting.py:169-237) with that channel's seeding threshold.  Results are those of correct_fov_image followed
 * by fit_fov_image movie by movie; what changes is the schedule: one library thread uploads movie k+1 while
 * `correct_threads` others run the corrections, drift and warps of the movies before it on streams of their own and one
 * more fits the channels of SEVERAL movies with one group fitter (fit_group_images images per group, see ia3_fit_fovs). */
#define IA3_MOVIE_MAXCH 8
typedef struct ia3_movie_params {
  int frames, X, Y;                    /* raw movie */
  int Z;                               /* planes per channel */
  int n_load;                          /* channels taken out of the movie (<= IA3_MOVIE_MAXCH) */
  int load_start[IA3_MOVIE_MAXCH];     /* first frame of each; frames start, start + load_step, ... */
  int load_step;                       /* number of colours in the movie */
  int n_sel;                           /* selected channels: corrected images / spot tables come back for these */
  int sel[IA3_MOVIE_MAXCH];            /* index into the loaded channels */
  int hot_pixel_corr; double hot_pixel_th;   /* io_tools/load.py:323-334 (hot_pix_th 0.5, float32 arithmetic) */
  int z_shift_corr;                    /* :337-345 */
  int n_bleed;                         /* :348-370: loaded channels mixed by the bleedthrough profile (0 = off) */
  int bleed_idx[IA3_MOVIE_MAXCH];      /* ... in the profile's channel order */
  const void* bleed_profile; int bleed_dtype;            /* device buffer (C,C,X,Y); 1 float32, 2 float64 */
  const void* illum_profile[IA3_MOVIE_MAXCH]; int illum_dtype[IA3_MOVIE_MAXCH];   /* per loaded channel, NULL = none (:373-384) */
  int drift_idx;                       /* loaded channel holding the beads; < 0: no drift measurement */
  const ia3_stack* ref_bead;           /* corrected reference bead stack, resident */
  ia3_drift_ref* drift_ref;            /* optional: a drift reference made from ref_bead and `crops` (else made per call) */
  int n_crops; int crops[8][3][2];     /* generate_drift_crops */
  int precision_fold, normalization, min_good_drifts; double drift_diff_th;
  int warp;                            /* 0: images are never resampled (warp_image=False, or a silent call: :434-436) */
  int warp_always[IA3_MOVIE_MAXCH];    /* per SELECTED channel: 1 = a chromatic channel, resampled whatever the drift;
                                          0 = resampled only when the drift is non-zero (:427) */
  const void* chrom_field[IA3_MOVIE_MAXCH]; int chrom_dtype[IA3_MOVIE_MAXCH];     /* per SELECTED channel: (3,Z,X,Y) device buffer or NULL */
  double highpass_sigma, highpass_truncate;   /* sigma <= 0: no high-pass */
  int fit_spots;
  ia3_seed_params seed[IA3_MOVIE_MAXCH];      /* per SELECTED channel (th_seed differs by channel, batch_functions.py:10-17) */
  ia3_fit_params fit;
  /* spot_tools/fitting.py:240-258: heights divided by the image's background level (1, normalize_background) or by the
   * level of each spot's neighbourhood of +-crop_size (2, normalize_local); bg_edges / bg_max_iter as in
   * ia3_find_background.  0 = heights as fitted. */
  int normalize; int bg_crop_size; const double* bg_edges; int bg_n_edges; int bg_max_iter;
  int correct_threads;                 /* <= 0: 2 */
  int fit_group_images;                /* <= 0: 12 */
  int upload_ahead;                    /* raw movies resident ahead of the corrections; <= 0: 2 */
} ia3_movie_params;
typedef struct ia3_movie_job {
  const void* host_raw;                /* (frames, X, Y) uint16 in host memory, or NULL to read `path` */
  const char* path; long long offset_bytes; int big_endian;
  double drift_in[3]; int measure_drift;      /* measure_drift 0: drift_in is used as it is (flag 0) */
  void* images_out[IA3_MOVIE_MAXCH];   /* per selected channel: host buffer for the corrected (Z,X,Y) uint16 image, or NULL */
  float* rows[IA3_MOVIE_MAXCH]; int capacity[IA3_MOVIE_MAXCH];      /* per selected channel: capacity x 11 float32 */
  /* out */
  double drift[3]; int drift_flag;
  int n_rows[IA3_MOVIE_MAXCH], n_seeds[IA3_MOVIE_MAXCH], n_iter[IA3_MOVIE_MAXCH];
  int rc;
  double t_upload_ms, t_correct_ms, t_fit_ms;   /* host wall time this movie spent in each stage */
  double stamps[6];   /* ms since the call began: upload begin / end, corrections begin / seeded, (last) group fit begin / end */
} ia3_movie_job;
int ia3_process_movies(ia3_movie_job* jobs, int n_jobs, const ia3_movie_params* p);

#ifdef __cplusplus
}
#endif
#endif /* IA3_H */
