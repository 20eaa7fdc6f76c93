"""GPU: the paired driver of the fit kernel (csrc/fit.hip, wave_gaussfit) — the two fits of a seed without neighbours run
together, the solver a half-wave each — against the same driver called once per fit (IA3_TUNE_FIT_PAIR=0), against two
work-list positions per seed (IA3_TUNE_FIT_FUSE=0), bit for bit, and against the oracle's rows.

Small stacks (24 x 64 x 64) with explicit seed lists through ia3_fit_create / ia3_fit_run / ia3_fit_results_ex; no seed
stage is involved."""
import ctypes as C
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPE = (24, 64, 64)
RTOL = 1e-4          # fit rows against the oracle, as tests/test_gpu_parity.py (assert_rows_close)
# centres of the eight spots: at least 13 voxels apart (balls of radius 5 do not touch), well inside the stack
SPOTS = np.array([[6.3, 10.2, 9.6], [7.1, 30.4, 11.2], [6.6, 50.7, 10.1], [12.4, 20.3, 31.8],
                  [17.2, 12.9, 52.3], [16.8, 33.5, 50.6], [17.5, 52.2, 51.4], [11.7, 44.1, 30.9]])


def make_stack(spots, seed=7, noise=12.0, bg=400.0, widths=None, shape=SHAPE, dh=300.0):
    """``widths``: (sz, sx, sy) of every spot (tests/harness/fitopt_cases.py); None: the widths of this module's spots;
    ``dh``: the step from one spot's height to the next's"""
    rng = np.random.RandomState(seed)
    z, x, y = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    im = bg + noise * rng.standard_normal(shape)
    for k, (cz, cx, cy) in enumerate(spots):
        h = 2500.0 + dh * k
        sz, sx, sy = (1.2 + 0.05 * k, 1.6, 1.7 - 0.04 * k) if widths is None else widths[k]
        im += h * np.exp(-0.5 * (((z - cz) / sz) ** 2 + ((x - cx) / sx) ** 2 + ((y - cy) / sy) ** 2))
    return np.clip(im, 1.0, 65000.0)


@pytest.fixture(scope="module")
def L():
    from imageanalysis3_amd import _lib
    _lib.check(_lib.lib().ia3_init(0))
    return _lib


@pytest.fixture(scope="module")
def stack_f32():
    return make_stack(SPOTS).astype(np.float32)


def run_fit(L, im, seeds, fp=None):
    """-> (rows (n, 11) float32, fits, nfev, sweeps) of one fitter on explicit seeds"""
    lib = L.lib()
    seeds = np.ascontiguousarray(seeds, dtype=np.float64)
    fp = L.make_fit_params() if fp is None else fp
    st = L.DeviceStack.upload(im)
    try:
        hh = C.c_void_p()
        L.check(lib.ia3_fit_create(st._h, L.dptr(seeds), len(seeds), C.byref(fp), C.byref(hh)))
        try:
            L.check(lib.ia3_fit_run(hh))
            ps = np.empty((len(seeds), 11), np.float32)
            it = C.c_int(0)
            L.check(lib.ia3_fit_results_ex(hh, L.ptr(ps), None, None, C.byref(it)))
            a, b = C.c_int64(0), C.c_int64(0)
            L.check(lib.ia3_fit_stats(hh, C.byref(a), C.byref(b)))
        finally:
            lib.ia3_fit_destroy(hh)
    finally:
        st.free()
    return ps, a.value, b.value, it.value


def three_ways(L, im, seeds, fp=None, maxfev=0):
    """the same fitter with the pair together, with one driver call per fit, and with two work-list positions per seed:
    tables (NaN rows by their bit pattern), fit and evaluation counts and sweep counts must agree; -> the paired run"""
    lib = L.lib()
    res = {}
    try:
        if maxfev:
            L.check(lib.ia3_set_tuning(L.IA3_DEBUG_FIT_MAXFEV, maxfev))
        for name, pair, fuse in (("pair", 1, 1), ("single", 0, 1), ("unfused", 1, 0)):
            L.check(lib.ia3_set_tuning(L.IA3_TUNE_FIT_PAIR, pair))
            L.check(lib.ia3_set_tuning(L.IA3_TUNE_FIT_FUSE, fuse))
            res[name] = run_fit(L, im, seeds, fp)
    finally:
        L.check(lib.ia3_set_tuning(L.IA3_TUNE_FIT_PAIR, 1))
        L.check(lib.ia3_set_tuning(L.IA3_TUNE_FIT_FUSE, 1))
        L.check(lib.ia3_set_tuning(L.IA3_DEBUG_FIT_MAXFEV, 0))
    ref = res["pair"]
    for name in ("single", "unfused"):
        got = res[name]
        print(name, "fits", got[1], "nfev", got[2], "sweeps", got[3], "| pair", ref[1:])
        assert np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32)), (name, got[0], ref[0])
        assert got[1:] == ref[1:], (name, got[1:], ref[1:])
    return ref


def oracle_rows(im, seeds, **kw):
    import np_oracle as O
    f = O.iter_fit_seed_points(im, np.asarray(seeds, dtype=np.float64).T, **kw)
    f.firstfit()
    f.repeatfit()
    return np.array(f.ps, dtype=np.float64), f


def assert_rows(got, ref):
    """row by row (same seed order), tolerances of tests/test_gpu_parity.py's assert_rows_close; NaN rows on both sides"""
    got = got.astype(np.float64)
    nan_g, nan_r = np.isnan(got).any(axis=1), np.isnan(ref).any(axis=1)
    assert np.array_equal(nan_g, nan_r), (nan_g, nan_r)
    a, b = got[~nan_g], ref[~nan_r]
    if len(a) == 0:
        return
    rel = np.abs(a[:, :8] - b[:, :8]) / np.abs(b[:, :8])
    assert rel.max() <= RTOL, ("max rel err %g at %s" % (rel.max(), np.unravel_index(rel.argmax(), rel.shape)))
    assert np.abs(a[:, 8:10] - b[:, 8:10]).max() <= 2e-3
    assert (np.abs(a[:, 10] - b[:, 10]) / np.abs(b[:, 10])).max() <= 1e-3


def seeds_of(spots, shift=(0, 1, 0)):
    return np.floor(np.asarray(spots)) + np.asarray(shift, dtype=np.float64)


def test_isolated_spots_f32(L, stack_f32):
    """every position is a pair: 2 fits per seed, one sweep"""
    seeds = seeds_of(SPOTS)
    ps, fits, nfev, sweeps = three_ways(L, stack_f32, seeds)
    assert fits == 2 * len(seeds) and not np.isnan(ps).any()
    assert np.abs(ps[:, 1:4] - SPOTS).max() < 0.2
    ref, f = oracle_rows(stack_f32, seeds)
    assert_rows(ps, ref)
    assert sweeps == f.n_iter


def test_isolated_spots_u16(L, stack_f32):
    """first-fit start point in integer arithmetic (kind 1) in one half, the refit's (kind 2) in the other"""
    im = np.round(stack_f32).astype(np.uint16)
    seeds = seeds_of(SPOTS)
    ps, fits, nfev, sweeps = three_ways(L, im, seeds)
    assert fits == 2 * len(seeds) and not np.isnan(ps).any()
    ref, f = oracle_rows(im, seeds)
    assert_rows(ps, ref)
    assert sweeps == f.n_iter


def test_isolated_and_overlapping_seeds(L):
    """two overlapping pairs of seeds (first fits and refits through the driver with one half empty) beside four
    isolated ones (pairs), in one launch"""
    spots = np.concatenate([SPOTS[:4], [[17.2, 12.9, 52.3], [17.9, 17.6, 50.2], [16.8, 44.5, 50.6], [14.5, 48.2, 47.4]]])
    im = make_stack(spots, seed=11).astype(np.float32)
    seeds = seeds_of(spots, (0, 0, 0))
    ps, fits, nfev, sweeps = three_ways(L, im, seeds)
    assert not np.isnan(ps).any()
    assert fits > 2 * len(seeds) - 1 and sweeps >= 1
    ref, f = oracle_rows(im, seeds)
    assert_rows(ps, ref)
    assert sweeps == f.n_iter


def test_pair_with_fits_that_stop_at_maxfev(L, stack_f32):
    """a seed on pure noise beside clean spots, at most 20 evaluations per fit: fits of a pair stop at the limit, the two
    halves finish rounds apart.  (No oracle rows: the reference's limit is not 20.)"""
    seeds = np.concatenate([seeds_of(SPOTS[:3]), [[12.0, 58.0, 30.0], [20.0, 30.0, 28.0]]])
    ps, fits, nfev, sweeps = three_ways(L, stack_f32, seeds, maxfev=20)
    assert fits == 2 * len(seeds)
    assert nfev <= 20 * fits
    free = run_fit(L, stack_f32, seeds)
    assert free[2] > nfev, (free[2], nfev)   # the limit did cut fits short


def test_clipped_balls(L, stack_f32):
    """a seed in the stack's corner whose clipped ball has fewer than ten voxels: no fit, NaN row (radius 1: 4 voxels);
    seeds on a face, an edge and in the corner at radius 5: partly filled voxel slots"""
    import np_oracle as O
    spots = np.array([[1.0, 1.3, 1.2], [0.8, 30.4, 11.2], [12.3, 0.9, 62.4], [6.3, 10.2, 9.6]])   # a spot under every seed
    im = make_stack(spots, seed=5).astype(np.float32)
    seeds = np.array([[0.0, 0.0, 0.0], [0.0, 30.0, 11.0], [12.0, 0.0, 63.0], [6.0, 10.0, 10.0]])
    zb, xb, yb = O.ball_offsets(1)
    z, x, y = O._in_dim(zb, xb, yb, *SHAPE)
    assert len(z) < 10
    fp = L.make_fit_params(radius_fit=1)
    ps, fits, nfev, sweeps = three_ways(L, im, seeds[:3], fp=fp)
    assert np.isnan(ps).all() and fits == 0 and nfev == 0
    ref, f = oracle_rows(im, seeds[:3], radius_fit=1)
    assert np.isnan(ref).all()
    ps, fits, nfev, sweeps = three_ways(L, im, seeds)
    assert fits == 2 * len(seeds)
    ref, f = oracle_rows(im, seeds)
    assert_rows(ps, ref)


def test_legacy_model_pair(L, stack_f32):
    """the legacy model (variant 1: per-axis start widths, its own centre map) through the same paired driver"""
    seeds = seeds_of(SPOTS)
    fp = L.make_fit_params(model_variant=1)
    ps, fits, nfev, sweeps = three_ways(L, stack_f32, seeds, fp=fp)
    assert fits == 2 * len(seeds) and not np.isnan(ps).any()
    # the oracle's legacy fitter with the same (default) options; tolerances of test_legacy_fit_single_image_golden
    import np_oracle as O
    f = O.iter_fit_seed_points_v3(stack_f32, seeds.T)
    f.firstfit()
    f.repeatfit()
    ref = np.array(f.ps, dtype=np.float64)
    np.testing.assert_allclose(ps[:, :8], ref[:, :8], rtol=RTOL, atol=1e-4)
    np.testing.assert_allclose(ps[:, 8:], ref[:, 8:], rtol=1e-3, atol=2e-3)
    assert sweeps == f.n_iter
