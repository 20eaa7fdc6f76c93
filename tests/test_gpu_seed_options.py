"""get_seeds off its defaults on the device: every window size, filter width and rule against the reference's own tables
(tests/golden/seedopt.npz) where the fixture holds the case and against the oracle otherwise, on the field of
tests/harness/seedopt_cases.py, which returns another table for every value of every option.

All comparisons are exact: a seed list is the set of its (z, x, y, h) rows, heights non-increasing.  The default
configuration (filt_size 3, widths 0.75 / 7.5, hot_pixel_th 3) is the business of tests/test_gpu_parity.py; here
* ``filt_size`` 1..8 runs the eight instantiations of seed_detect<T, ZC, W>, whose window is lopsided for an even W;
* the front and background widths switch the lazy / fused detector on and off (background radius 3 | 4, 63 | 64), flip its
  bound's block size (32 | 33) and make gauss_dog_pair decline (front radius other than 3);
* ``hot_pixel_th`` 0..6 and ``min_edge_distance`` 0..13 run through the fused and the dense detector and through both
  finishes: on the device (fin_*_k) and, above FIN_CAP candidates, on the host (finish_seeds).
"""
import ctypes as C

import numpy as np
import pytest
from conftest import load_golden

from harness import seedopt_cases as K
from test_gpu_parity import seed_set

pytestmark = pytest.mark.gpu

DTYPES = list(K.DTYPES)
_gold = {}
_oracle = {}
_by_options = {(name, tuple(sorted(kw.items()))): key for key, (name, kw) in K.golden_cases().items()}


def want(name, dtype, **kw):
    """The reference's table where the fixture has the case, the oracle's otherwise; made once."""
    opts = tuple(sorted(kw.items()))
    key = _by_options.get((name, opts))
    if key is not None:
        if not _gold:
            _gold.update(load_golden("seedopt.npz"))
            for n in ("main", "ragged", "noise"):
                for dt in DTYPES:
                    assert np.uint32(K.crc(K.stack(n, dt))) == _gold["crc_%s_%s" % (n, dt)], (n, dt)
        return K.golden_table(_gold, dtype, key)
    if (name, dtype, opts) not in _oracle:
        import np_oracle as O
        _oracle[(name, dtype, opts)] = O.get_seeds(np.array(K.stack(name, dtype)), return_h=True, **kw)
    return _oracle[(name, dtype, opts)]


def same(got, ref, what):
    assert got.dtype == np.float64 and got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(seed_set(got), seed_set(ref)), what
    assert (np.diff(got[:, 3]) <= 0).all(), what                 # brightest first


def seeds(name, dtype, **kw):
    from imageanalysis3_amd.spot_tools.fitting import get_seeds
    return get_seeds(np.array(K.stack(name, dtype)), return_h=True, **kw)


def check(name, dtype, **kw):
    got = seeds(name, dtype, **kw)
    same(got, want(name, dtype, **kw), (name, dtype, kw))
    return got


def fused_units():
    """(tile, plane) units of this thread's last seed stage: above 0 exactly when the fused detector ran."""
    from imageanalysis3_amd import _lib as L
    out = (C.c_double * 2)()
    L.check(L.lib().ia3_seed_skip_stats(out))
    return out[1]


def seed_dense(on):
    from imageanalysis3_amd import _lib as L
    L.check(L.lib().ia3_set_tuning(L.IA3_TUNE_SEED_DENSE, 1 if on else 0))


# ---- windows -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gfilt_size", K.FRONT_WIDTHS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_window_size(dtype, gfilt_size):
    tables = [check("main", dtype, **dict(K.BASE, filt_size=W, gfilt_size=gfilt_size)) for W in K.FILT_SIZES]
    assert len({K.as_set(t) for t in tables}) == len(K.FILT_SIZES)   # equal to eight different tables: W is not ignored


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_window_size_ragged(dtype):
    for g in (0, 0.75):
        tables = [check("ragged", dtype, **dict(K.BASE, filt_size=W, gfilt_size=g)) for W in K.FILT_SIZES]
        assert len({K.as_set(t) for t in tables}) == len(K.FILT_SIZES)


@pytest.mark.parametrize("dtype", DTYPES)
def test_even_window_is_lopsided(dtype):
    """Of the twins at distance W / 2 from their brighter spike, the one below it is dropped and the one above it kept."""
    for W in (2, 4, 6, 8):
        zxy = {tuple(int(v) for v in r[:3]) for r in seeds("main", dtype, **dict(K.BASE, filt_size=W, gfilt_size=0))}
        for (ax, d, s), _, dim in K.pairs(K.MAIN_SHAPE):
            if d == W // 2:
                assert (dim in zxy) == (s < 0), (W, ax, s)


def test_unsupported_window_on_a_resident_stack():
    from imageanalysis3_amd import _lib as L
    from imageanalysis3_amd.spot_tools.fitting import get_seeds
    with L.DeviceStack.upload(np.array(K.stack("ragged", "uint16"))) as st:
        for W in (0, 9):
            with pytest.raises(NotImplementedError, match=r"filt_size %d not in 1\.\.8" % W):
                get_seeds(st, th_seed=500, filt_size=W)


# ---- filters -------------------------------------------------------------------------------------------------------------
FILTERS = [dict(gfilt_size=0), dict(gfilt_size=0.5), dict(gfilt_size=1.0), dict(gfilt_size=1.5)] + \
          [dict(background_gfilt_size=b, th_seed=K.BACK_OFF_TH if b < 0.75 else 500) for b in K.BACK_WIDTHS] + \
          [dict(gfilt_size=0, background_gfilt_size=0, th_seed=K.BACK_OFF_TH),
           dict(gfilt_size=1.5, background_gfilt_size=8.2), dict(gfilt_size=0, background_gfilt_size=15.7)]


@pytest.mark.parametrize("dtype", DTYPES)
def test_filter_widths(dtype):
    for f in FILTERS:
        got = check("main", dtype, **dict(K.BASE, **f))
        assert len(got) >= 10, f


# ---- rules ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt_size", [3, 5])
@pytest.mark.parametrize("dtype", DTYPES)
def test_hot_pixel_thresholds(dtype, filt_size):
    counts = []
    for t in K.HOT_THS:
        kw = dict(K.BASE, remove_hot_pixel=True, hot_pixel_th=t)
        if filt_size != 3:
            kw["filt_size"] = filt_size
        counts.append(len(check("main", dtype, **kw)))
        assert (fused_units() > 0) == (filt_size == 3)      # default filters, Y % 32 == 0, Z = 25: the fused detector
    assert counts[0] == counts[1] == 0 and len(set(counts[1:])) == 6, counts
    check("main", dtype, **dict(K.BASE, remove_hot_pixel=True, hot_pixel_th=2.5, filt_size=filt_size))    # counts >= 2.5


@pytest.mark.parametrize("filt_size", [3, 5])
@pytest.mark.parametrize("dtype", DTYPES)
def test_edge_distances(dtype, filt_size):
    counts = {}
    for d in (0, 1, 2, 2.5, 3, 5, 7, 13):
        kw = dict(K.BASE, min_edge_distance=d)
        if filt_size != 3:
            kw["filt_size"] = filt_size
        counts[d] = len(check("main", dtype, **kw))
    assert counts[2.5] == counts[3] != counts[2] and counts[13] == 0, counts
    assert len({counts[d] for d in (0, 1, 2, 3, 5, 7)}) == 6, counts


@pytest.mark.parametrize("dtype", DTYPES)
def test_max_num_seeds_with_other_windows(dtype):
    for W, g, n in ((2, 0, 40), (4, 0.75, 25), (5, 0.75, 100), (6, 1.0, 1)):
        kw = dict(K.BASE, filt_size=W, gfilt_size=g)
        full = want("main", dtype, **kw)
        assert n == len(full) or n > len(full) or full[n - 1, 3] > full[n, 3]      # the cut goes through no tie
        got = seeds("main", dtype, max_num_seeds=n, **kw)
        same(got, full[:n], (dtype, W, g, n))


@pytest.mark.parametrize("dtype", DTYPES)
def test_dynamic_threshold_settles_on_a_middle_level(dtype):
    got = check("main", dtype, **K.DYNAMIC)
    th = K.DYNAMIC["th_seed"] * (1 - K.DYNAMIC_LEVEL / K.DYNAMIC["dynamic_niters"])
    above = K.DYNAMIC["th_seed"] * (1 - (K.DYNAMIC_LEVEL - 1) / K.DYNAMIC["dynamic_niters"])
    assert len(got) >= K.DYNAMIC["min_dynamic_seeds"] > (got[:, 3] >= above).sum() and got[:, 3].min() >= th
    check("main", dtype, **dict(K.DYNAMIC, filt_size=4, min_dynamic_seeds=50))
    check("main", dtype, **dict(K.DYNAMIC, remove_hot_pixel=True, hot_pixel_th=2, min_edge_distance=2.5))


# ---- both finishes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_both_finishes_follow_the_same_rule(dtype):
    """The same window, filters and hot-column thresholds where the host finishes the list (finish_seeds: more candidates
    than FIN_CAP on the noise stack; on the field at threshold 0 fewer, but more at the chosen level than the device finish
    packs) and where the device does (fin_*_k: the field at threshold 500).  ``hot_pixel_th=0``: every column holds at least
    0 seeds, so the reference drops them all."""
    opts = dict(K.BASE, filt_size=2, gfilt_size=0)
    cases = (("noise", -1e3), ("main", 0), ("main", 500))
    n = [len(want(name, dtype, **dict(opts, th_seed=th))) for name, th in cases]
    assert n[0] > K.FIN_CAP > n[1] > K.FIN_KEYS > 64 * n[2] > 0, n
    for name, th in cases:
        check(name, dtype, **dict(opts, th_seed=th))
        for t in (0, 2, 5):
            got = check(name, dtype, **dict(opts, th_seed=th, remove_hot_pixel=True, hot_pixel_th=t))
            assert (len(got) == 0) == (t == 0), (name, t)


# ---- every entry ---------------------------------------------------------------------------------------------------------
ENTRY_OPTIONS = [dict(filt_size=2, gfilt_size=0), dict(filt_size=5), dict(filt_size=8, gfilt_size=1.0),
                 dict(remove_hot_pixel=True, hot_pixel_th=2), dict(remove_hot_pixel=True, hot_pixel_th=0),
                 dict(min_edge_distance=2.5), dict(background_gfilt_size=0.9), dict(background_gfilt_size=8.2),
                 dict(gfilt_size=0, filt_size=4, min_edge_distance=3, remove_hot_pixel=True, hot_pixel_th=4)]
CROP = dict(sel_center=(12, 38, 48), seed_radius=15)


@pytest.mark.parametrize("dense", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_entry_takes_the_options(dtype, dense):
    from imageanalysis3_amd import _lib as L
    from imageanalysis3_amd.spot_tools.fitting import get_seeds
    im = np.array(K.stack("main", dtype))
    lo, hi = np.array(CROP["sel_center"]) - CROP["seed_radius"], np.array(CROP["sel_center"]) + CROP["seed_radius"]
    inside = lambda p: bool(((np.array(p) >= lo) & (np.array(p) < hi)).all())   # noqa: E731
    assert sum(inside(b) != inside(d) for _, b, d in K.pairs(K.MAIN_SHAPE)) >= 2   # the crop cuts through pairs
    seed_dense(dense)
    try:
        with L.DeviceStack.upload(im) as st:
            for o in ENTRY_OPTIONS:
                kw = dict(K.BASE, **o)
                ref, ref_crop = want("main", dtype, **kw), want("main", dtype, **dict(kw, **CROP))
                same(get_seeds(im, return_h=True, **kw), ref, ("ndarray", o))
                same(get_seeds(st, return_h=True, **kw), ref, ("resident", o))
                same(get_seeds(im, return_h=True, **kw, **CROP), ref_crop, ("ndarray crop", o))
                same(get_seeds(st, return_h=True, **kw, **CROP), ref_crop, ("resident crop", o))
                assert len(ref) == 0 or 0 < len(ref_crop) < len(ref), o
                assert get_seeds(st, **kw).shape == (len(ref), 3)
    finally:
        seed_dense(0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_fit_fov_image_hands_the_options_on(dtype):
    from imageanalysis3_amd.spot_tools.fitting import fit_fov_image, get_seeds
    im = np.array(K.stack("main", dtype))
    top = dict(th_seed=500, use_dynamic_th=False, remove_hot_pixel=True)
    rows = lambda t: t[np.lexsort(t.T[::-1])]   # noqa: E731
    for o in (dict(filt_size=5, min_edge_distance=2.5, hot_pixel_th=4), dict(filt_size=2, gfilt_size=1.0, hot_pixel_th=2),
              dict(background_gfilt_size=8.2, min_edge_distance=5)):
        s = get_seeds(im, return_h=True, **top, **o)
        same(s, want("main", dtype, **top, **o), o)
        a = fit_fov_image(im, "647", max_num_seeds=None, seeding_kwargs=o, verbose=False, **top)
        b = fit_fov_image(im, "647", seeds=s, verbose=False)
        assert a.ndim == 2 and a.shape == b.shape and a.shape[1] == 11 and len(a) > 0, (o, a.shape, b.shape)
        assert np.array_equal(rows(a), rows(b)), o


# ---- legacy rule ---------------------------------------------------------------------------------------------------------
def _tie_canon(s):
    s = np.asarray(s)
    return s[np.lexsort((s[:, 2], s[:, 1], s[:, 0], -s[:, 3]))] if len(s) else s.reshape(0, 4)


def test_legacy_seeding_with_other_windows():
    """visual_tools.get_seed_points_base / get_seed_in_distance (rule 1 of the generic detector) on the uint16 field."""
    import np_oracle as O
    from imageanalysis3_amd import visual_tools as vt
    im = np.array(K.stack("main", "uint16"))
    tables = []
    for W in (2, 4, 5):
        for bg, hot in ((10, 0), (10, 2), (5, 3)):
            got = vt.get_seed_points_base(im, 0.75, bg, W, 500, hot, True)
            ref = O.legacy_get_seed_points_base(im, 0.75, bg, W, 500, hot, True)
            assert got.dtype == np.int64 and got.shape == ref.shape and ref.shape[1] > 20, (W, bg, hot, got.shape, ref.shape)
            assert np.array_equal(got, ref), (W, bg, hot)
        tables.append(K.as_set(got.T))
        for center, dynamic in (([12, 38, 48], True), ([12, 38, 48], False), (None, False)):
            args = (center, 0, 20, 0.75, 10, W, False, 95, 500, dynamic, 10, 2, 1, 4, True)
            got, ref = vt.get_seed_in_distance(im, *args), O.legacy_get_seed_in_distance(im, *args)
            assert got.dtype == np.int64 and got.shape == ref.shape and len(ref) > 5, (W, center, dynamic, got.shape, ref.shape)
            assert np.array_equal(got[:, 3], ref[:, 3]), (W, center, dynamic)
            assert np.array_equal(_tie_canon(got), _tie_canon(ref)), (W, center, dynamic)
    assert len(set(tables)) == 3
