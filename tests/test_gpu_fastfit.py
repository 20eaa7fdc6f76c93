"""GPU: the Fitting_v4 fast path on the device (fastfit.hip) against the reference's own results
(tests/golden/fastfit.npz, scripts/make_fastfit_golden.py) and, on other inputs, against the NumPy statement
tests/harness/fastfit_ref.py, which tests/test_fastfit_cpu.py holds to the same goldens bit for bit.

Exact: seed sets and heights, every column of the moment-fit rows (NaNs included), normalzie_im.  np.std: the device
sums in float64 and rounds to NumPy's output dtype, NumPy sums a float32 stack in float32; the generator recorded
|np.std(x) - np.std(float64(x))| / std per fixture (fastfit.json) and asserted that no voxel lies that close to a cutoff;
the test allows four times the largest recorded value.  better_fit rows: the project's 1e-4 relative bar on the first
eight columns (tests/test_gpu_parity.py)."""
import json
import os

import numpy as np
import pytest

from conftest import load_golden
from harness import fastfit_ref as FR
from imageanalysis3_amd._lib import IA3_TUNE_FIT_NBLIST

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
META = json.load(open(os.path.join(HERE, "golden", "fastfit.json")))


@pytest.fixture(scope="module")
def gold():
    return load_golden("fastfit.npz")


def _same(a, b):
    """Same shape, dtype and bits; a NaN matches a NaN whatever its sign and payload (0/0 gives -nan on the host that
    made the fixtures and +nan on the device: IEEE 754 leaves both open)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return a.tobytes() == b.tobytes()
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.where(na, 0, a).tobytes() == np.where(nb, 0, b).tobytes()


def _kw(run):
    return {k: v for k, v in run.items() if k != "n"}


@pytest.mark.parametrize("key", sorted(META["seed_runs"]))
def test_seeds_equal_reference(gold, key):
    from imageanalysis3_amd.External.Fitting_v4 import get_seed_points_base_v2
    run = _kw(META["seed_runs"][key])
    im = gold[key.split("_")[0] + "_im"]
    got, std_ = get_seed_points_base_v2(im, **run)
    want, wstd = gold[key], gold[key + "_std"]
    rel = abs(float(std_) - float(wstd)) / float(wstd)
    print(key, "seeds", got.shape[1], "std rel diff %.3g" % rel, "band %.3g" % META["std_band"])
    assert META["std_band"] == META["std_band_factor"] * max(META["std_rel_diff"].values())
    assert std_.dtype == wstd.dtype and rel <= META["std_band"]
    assert _same(got, want)
    # the same voxel tests against the statement run with the device's own std_
    mine, _ = FR.seeds(im, run["gfilt_size"], run["filt_size"], run["th_seed"], run["max_num"], std=std_)
    assert _same(got, mine)
    again, std2 = get_seed_points_base_v2(im, **run)
    assert _same(again, got) and _same(std2, std_)


@pytest.mark.parametrize("case", ["c1", "c2", "c3"])
def test_normalzie_im_equals_statement_and_reference(gold, case):
    from imageanalysis3_amd import _lib as L
    from imageanalysis3_amd.External.Fitting_v4 import normalzie_im
    im = gold[case + "_im"]
    got = normalzie_im(im)
    assert _same(got, gold[case + "_norm20"]) and _same(got, FR.normalise(im, 20))
    for sz in (1, 3, 32):
        assert _same(normalzie_im(im, sz), FR.normalise(im, sz)), sz
    with L.DeviceStack.upload(im) as s, normalzie_im(s, 7) as out:
        assert isinstance(out, L.DeviceStack) and out.dtype == np.float32 and _same(out.download(), FR.normalise(im, 7))
    with pytest.raises(NotImplementedError):
        normalzie_im(im, 33)


@pytest.mark.parametrize("key", sorted(k for k, r in META["fit_runs"].items() if not r.get("better_fit")))
def test_moment_rows_equal_reference_bit_for_bit(gold, key):
    from imageanalysis3_amd.External.Fitting_v4 import fast_fit_big_image
    case = key.split("_")[0]
    im, cen = gold[case + "_im"], gold[case + "_centres"]
    got = fast_fit_big_image(im, cen, **_kw(META["fit_runs"][key]))
    want = gold[key]
    bad = np.argwhere(got.view(np.uint64) != want.view(np.uint64)) if got.shape == want.shape else None
    assert _same(got, want), (key, bad)
    assert _same(fast_fit_big_image(im, cen, **_kw(META["fit_runs"][key])), got)     # identical bytes on a second call
    assert _same(fast_fit_big_image(im, cen, verbose=False, **_kw(META["fit_runs"][key])), got)


def test_better_fit_rows_meet_the_project_bar(gold):
    from imageanalysis3_amd.External.Fitting_v4 import fast_fit_big_image
    want = gold["c1_fit_better"]
    got = fast_fit_big_image(gold["c1_im"], gold["c1_centres"], better_fit=True)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32 and np.all(np.isfinite(want))
    rel = np.abs(got[:, :8].astype(np.float64) - want[:, :8]) / np.abs(want[:, :8])
    print("better_fit max rel err %.3g over %d rows" % (rel.max(), len(want)))
    assert rel.max() <= 1e-4


def test_gfit_fast_equals_reference(gold):
    from imageanalysis3_amd.External.Fitting_v4 import gfit_fast
    vals, X = gold["gf_vals"], gold["gf_X"]
    u16 = gold["c3_im"][3:7, 18:23, 20:24].ravel()
    assert _same(gfit_fast(vals, X), gold["gf_plain"])
    assert _same(gfit_fast(vals, X, bk_f=0.3), gold["gf_bk03"])
    assert _same(gfit_fast(vals.astype(np.float64), X), gold["gf_f64"])
    assert _same(gfit_fast(u16, X), gold["gf_u16"])
    assert _same(gfit_fast(vals, X, reconstruct=True), gold["gf_recon"])
    assert _same(gfit_fast(vals[:0], X[:, :0]), gold["gf_empty"])
    # every list length at which the summation takes another path (ia3_npsum.h), against the statement
    rng = np.random.default_rng(3)
    for n in (1, 7, 8, 9, 63, 64, 65, 128, 129, 254, 263, 490, 511, 512):
        v = rng.normal(500., 80., n).astype(np.float32)
        x = rng.integers(0, 40, (3, n))
        assert _same(gfit_fast(v, x), FR.moments(v, x)), n
    with pytest.raises(NotImplementedError):
        gfit_fast(np.ones(513, np.float32), np.zeros((3, 513), int))


def _crowded_field(shape, n, seed, integer):
    """n centres: half in one tight blob (more than 64 neighbours each at any supported radius), the rest spread over the
    stack; then a centre outside the image (a NaN row), one on the far corner and one in the first voxel."""
    rng = np.random.default_rng(seed)
    lo, hi = np.array([1., 4., 4.]), np.array(shape) - np.array([1., 4., 4.])
    blob = rng.normal([shape[0] / 2, shape[1] / 3, shape[2] / 3], [1.0, 1.5, 1.5], (n // 2, 3))
    rest = rng.uniform(lo, hi, (n - n // 2, 3))
    cen = np.concatenate([blob, rest])
    cen = np.floor(cen) if integer else cen
    extra = [[-8., 5., 5.], [shape[0] - 0.5, shape[1] - 0.5, shape[2] - 0.1], [0.2, 0.3, 0.4]]
    return np.concatenate([cen, np.array(extra)])


@pytest.mark.parametrize("dtype,radius,integer", [(np.float32, 4, True), (np.float32, 4, False), (np.uint16, 3, False),
                                                  (np.float32, 5, False), (np.float32, 2, True)])
def test_moment_rows_equal_statement_on_crowded_fields(dtype, radius, integer):
    """A 9 x 37 x 67 stack (no multiple of anything), 303 centres, half of them in one blob (more than 64 neighbours:
    the scan path; duplicates and exact ties among the integer centres), the rest spread out, one outside the image."""
    from imageanalysis3_amd import _lib as L, synth
    from imageanalysis3_amd.External.Fitting_v4 import fast_fit_big_image
    shape = (9, 37, 67)
    im, _, _ = synth.make_fov(shape, 6, 77, dtype=dtype, margin=(2, 6, 6), min_sep=6.0)
    cen = _crowded_field(shape, 300, 5 + radius, integer)
    d = np.sqrt(((cen[:, None] - cen[None]) ** 2).sum(-1))
    assert ((d <= 2 * radius).sum(1) - 1).max() > 64 and ((d <= 2 * radius).sum(1) - 1).min() <= 64
    for kw in ({}, {"recenter": True}, {"avoid_neigbors": False}):
        want = FR.fast_fit(im, cen, radius_fit=radius, **kw)
        got = fast_fit_big_image(im, cen, radius_fit=radius, **kw)
        assert _same(got, want), (kw, np.argwhere(got.view(np.uint64) != want.view(np.uint64))[:5])
    assert np.isnan(want[-3]).all() and np.isfinite(want[:, :11]).all(1).sum() > 150
    with L.DeviceStack.upload(im) as s:
        assert _same(fast_fit_big_image(s, cen, radius_fit=radius, avoid_neigbors=False), got)


def test_neighbour_scan_equals_neighbour_list(gold):
    """IA3_TUNE_FIT_NBLIST lowered to 0: every seed with a neighbour scans the seed list instead of reading its list."""
    from imageanalysis3_amd import _lib as L
    from imageanalysis3_amd.External.Fitting_v4 import fast_fit_big_image
    runs = [(gold["c2_im"], gold["c2_centres"]), (gold["c1_im"], _crowded_field((12, 40, 44), 150, 21, True))]
    listed = [fast_fit_big_image(im, cen) for im, cen in runs]
    try:
        L.check(L.lib().ia3_set_tuning(IA3_TUNE_FIT_NBLIST, 0))
        scanned = [fast_fit_big_image(im, cen) for im, cen in runs]
    finally:
        L.check(L.lib().ia3_set_tuning(IA3_TUNE_FIT_NBLIST, 64))
    for a, b in zip(listed, scanned):
        assert _same(a, b)
    assert _same(listed[0], gold["c2_fit_default"])
    assert _same(listed[1], FR.fast_fit(gold["c1_im"], runs[1][1]))


@pytest.mark.parametrize("shape", [(2, 5, 70), (5, 9, 129), (7, 4, 64)])
def test_seeds_equal_statement_on_small_and_ragged_stacks(shape):
    """Axes shorter than the neighbourhood (the wrapped index passes the same voxel more than once), ragged tiles,
    more than one tile along y; every supported neighbourhood; uint16 and float32; equal values (plateaus are kept)."""
    from imageanalysis3_amd.External.Fitting_v4 import get_seed_points_base_v2
    rng = np.random.default_rng(shape[2])
    f32 = rng.normal(0., 1., shape).astype(np.float32)
    u16 = rng.integers(0, 12, shape).astype(np.uint16)      # many equal neighbours
    for im, th in ((f32, 1.5), (u16, 0.5)):
        for filt_size in (1, 3, 5, 7):
            got, std_ = get_seed_points_base_v2(im, gfilt_size=0, filt_size=filt_size, th_seed=th)
            want, wstd = FR.seeds(im, 0, filt_size, th, std=std_)
            # a float64-accurate value rounded to float32 lies within half a float32 ulp of the float64 one: eps covers it
            exact = float(np.std(im.astype(np.float64)))
            assert abs(float(std_) - exact) <= float(np.finfo(np.float32).eps) * exact and std_.dtype == np.std(im).dtype
            # equal heights: the order among them is not the reference's to define (an unstable argsort); compare as sets
            assert got.dtype == want.dtype and got.shape == want.shape, (shape, filt_size)
            assert sorted(map(tuple, got.T)) == sorted(map(tuple, want.T)), (shape, filt_size)
            assert np.all(np.diff(got[3]) <= 0)
    got, sd = get_seed_points_base_v2(f32, gfilt_size=3, filt_size=3, th_seed=1.0, max_num=5)
    want, _ = FR.seeds(f32, 3, 3, 1.0, 5, std=sd)
    assert _same(got, want) and got.shape == (4, 5)
    # a NumPy float64 threshold makes the cutoff and the comparison float64
    got64, sd = get_seed_points_base_v2(f32, gfilt_size=0, th_seed=np.float64(1.5))
    want64, _ = FR.seeds(f32, 0, 3, np.float64(1.5), std=sd)
    assert _same(got64, want64)
