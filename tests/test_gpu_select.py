"""GPU: the one radix select (csrc/ia3_select.h) through every public entry point that runs it, on the shapes and values
where its parts can go wrong: plane_medians and stack_median (morph.hip, chromim.hip), order_stats (stats.hip), the
medians of ia3_z_shift_correction (corrections.hip) and the float64 front of find_candidate_chromosomes.  Every result is
compared with np.sort / np.median with == (NaN where NaN is the answer)."""
import ctypes as C
import warnings

import numpy as np
import pytest
from scipy import ndimage
from scipy.stats import scoreatpercentile

pytestmark = pytest.mark.gpu

DTYPES = (np.uint16, np.float32)


@pytest.fixture(scope="module")
def L():
    from imageanalysis3_amd import _lib
    _lib.check(_lib.lib().ia3_init(0))
    return _lib


def eq(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    assert np.array_equal(got, want, equal_nan=True), (got, want)


def medians(a):
    """np.median of every plane and of the whole stack, in the dtype NumPy gives them"""
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        return np.array([np.median(p) for p in a] + [np.median(a)])


def zshift_medians(L, im):
    out = np.empty(im.shape, np.uint16)
    med = np.empty(im.shape[0] + 1, np.float32)
    L.check(L.lib().ia3_z_shift_correction(L.ptr(im), L.dtype_code(im), im.shape[0], im.shape[1], im.shape[2], L.ptr(out),
                                           med.ctypes.data_as(C.POINTER(C.c_float))))
    return med


def some_ranks(n):
    return np.unique(np.clip([0, 1, n // 4, (n - 1) // 2, n // 2, 3 * n // 4, n - 2, n - 1], 0, n - 1)).astype(np.int64)


def check_all(L, im, zshift=True):
    im = np.ascontiguousarray(im)
    want = medians(im)
    with L.DeviceStack.upload(im) as dev:
        eq(L.plane_medians(dev), want[:-1].astype(np.float64))
        got = L.stack_median(dev)
        assert type(got) is np.float64
        eq(got, np.float64(want[-1]))
        ranks = some_ranks(im.size)
        eq(dev.order_stats(ranks), np.sort(im, axis=None)[ranks])
        eq(dev.download(), im)
    if zshift:   # the z-shift takes its medians of the stack as float32 (a float32 stack that holds NaN is outside its contract)
        eq(zshift_medians(L, im), medians(im.astype(np.float32)))


def hi8(a):
    """the most significant byte of the select's key: what pass 0 sorts by"""
    if a.dtype == np.uint16:
        return a >> 8
    b = a.view(np.uint32)
    return np.where(b >> 31 != 0, ~b, b | np.uint32(1 << 31)) >> 24


def spread(rng, dt, shape, lo, hi):
    return rng.integers(lo, hi, shape).astype(dt) if dt == np.uint16 else (rng.random(shape) * (hi - lo) + lo).astype(dt)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", [(4, 1, 1), (5, 1, 3), (3, 5, 7), (130, 3, 3)])
def test_short_and_unaligned_segments_and_many_planes(L, dt, shape):
    """Planes of 1, 3 and 35 voxels start off the 16-byte boundaries and are shorter than a vector or end in a tail; 130
    planes (131 problems with the whole stack) take more than one block of the pick kernel."""
    rng = np.random.default_rng(sum(shape))
    check_all(L, spread(rng, dt, shape, 0, 65536))
    check_all(L, spread(rng, dt, shape, 300, 303))           # ties


@pytest.mark.parametrize("dt", DTYPES)
def test_ranks_that_part_at_the_first_pass_beside_one_group(L, dt):
    """Plane 0: half the voxels in the lowest key byte, half in the highest, so its two middle ranks part at pass 0; plane 1
    is constant: one group to the end."""
    rng = np.random.default_rng(5)
    im = np.empty((2, 4, 8), dt)
    lo = spread(rng, dt, 16, 0, 256) if dt == np.uint16 else -spread(rng, dt, 16, 2.0e38, 3.0e38)
    hi = spread(rng, dt, 16, 65280, 65536) if dt == np.uint16 else spread(rng, dt, 16, 2.0e38, 3.0e38)
    im[0] = rng.permutation(np.concatenate([lo, hi])).reshape(4, 8)
    im[1] = 1000
    assert hi8(lo).max() == 0 and hi8(hi).min() == 255
    check_all(L, im)
    check_all(L, im[::-1])


@pytest.mark.parametrize("dt", DTYPES)
def test_union_groups_that_no_plane_has(L, dt):
    """Planes alternate between two disjoint ranges, three of the upper and two of the lower: the whole stack's middle ranks
    lie low in the upper range, in a key byte that no plane's middle ranks share."""
    rng = np.random.default_rng(6)
    im = np.empty((5, 16, 16), dt)
    for z in range(5):
        im[z] = spread(rng, dt, (16, 16), 30000, 60000) if z % 2 == 0 else spread(rng, dt, (16, 16), 100, 5000)
    if dt == np.float32:
        im = np.exp2(im / np.float32(3000.0)).astype(dt)   # over several binades: the key byte is the exponent's
    s = np.sort(im, axis=None)
    mid = hi8(s[[(im.size - 1) // 2, im.size // 2]])
    planes = np.concatenate([hi8(np.sort(p, axis=None)[[127, 128]]) for p in im])
    assert not np.isin(mid, planes).any(), (mid, planes)
    check_all(L, im)


@pytest.mark.parametrize("dt", DTYPES)
def test_sixteen_ranks(L, dt):
    rng = np.random.default_rng(7)
    im = spread(rng, dt, (3, 5, 7), 0, 65536)
    ranks = np.array([0, 104, 52, 52, 0, 104, 1, 2, 3, 50, 51, 53, 103, 7, 7, 99], np.int64)
    with L.DeviceStack.upload(im) as dev:
        eq(dev.order_stats(ranks), np.sort(im, axis=None)[ranks])
        eq(dev.order_stats(np.full(16, 104)), np.full(16, im.max()))
        with pytest.raises(ValueError, match="at most 16 ranks"):
            dev.order_stats(np.zeros(17, np.int64))


def test_nan_in_exactly_one_plane(L):
    rng = np.random.default_rng(8)
    im = spread(rng, np.float32, (4, 5, 7), 1, 1000)
    clean = medians(im)
    for z, sign in ((2, 1), (0, -1), (3, 1)):
        bad = im.copy()
        bad[z, 3, 4] = np.copysign(np.nan, sign)
        want = clean.copy()
        want[[z, -1]] = np.nan
        assert np.array_equal(medians(bad), want, equal_nan=True)
        check_all(L, bad, zshift=False)


def test_nan_in_exactly_one_float64_plane(L):
    """The float64 front names the first plane whose median it cannot divide by and that median, which is all it shows of
    its plane medians when it refuses an image: the planes before the NaN plane are untouched (all others when the NaN is
    in the last plane), an infinite plane before the NaN plane keeps its own median, and the clean image gives NumPy's
    threshold.  Planes after the NaN plane cannot be seen through this entry; plane_medians shows them for float32."""
    from imageanalysis3_amd.segmentation_tools import chromosome as CH
    rng = np.random.default_rng(9)
    im = rng.random((4, 10, 12)) + 1.0
    adj = np.array([p / np.median(p) for p in im])
    seed = ndimage.maximum_filter(adj, 3, mode='nearest') - ndimage.minimum_filter(adj, 3, mode='nearest')
    with L.ChromImage.upload(im) as dev:
        assert L.find_candidate_chromosomes(dev, 3, 90., 1, 1)[1] == scoreatpercentile(seed, 90.)
    for z in (2, 0, 3):
        bad = im.copy()
        bad[z, 1, 5] = np.nan
        with L.ChromImage.upload(bad) as dev:
            with pytest.raises(ValueError, match="plane %d has the median nan" % z):
                CH.find_candidate_chromosomes(dev, _verbose=False)
    bad = im.copy()
    bad[1] = np.inf                                               # refused for its own median, not for plane 3's NaN
    bad[3, 1, 5] = np.nan
    with L.ChromImage.upload(bad) as dev:
        with pytest.raises(ValueError, match="plane 1 has the median inf"):
            CH.find_candidate_chromosomes(dev, _verbose=False)


def test_zeros_infinities_and_denormals_in_the_middle(L):
    d = np.float32(1e-45)                                       # the smallest float32 denormal
    inf = np.float32(np.inf)
    even = np.array([[-1, -0.0, 0.0, 1], [-1, 0.0, -0.0, 1], [-inf, -inf, inf, inf], [0, inf, inf, inf], [-inf, -inf, -inf, 0],
                     [0, d, 3 * d, 1], [-1, -3 * d, -d, 0], [-d, -0.0, 0.0, d], [-inf, -d, d, inf]], np.float32)
    odd = np.array([[-1, -0.0, 1], [-1, 0.0, 1], [-inf, inf, inf], [-inf, -inf, inf], [-1, d, 1], [-1, -d, 1], [-d, 0, d]], np.float32)
    assert d > 0 and d / 2 == 0
    rng = np.random.default_rng(10)
    for rows in (even, odd):
        check_all(L, rng.permuted(rows, axis=1)[:, None, :])


def test_float64_denormals_zeros_and_infinities_in_the_middle(L):
    """The float64 front shows its plane medians in two ways: the threshold it returns (every plane is divided by its
    median first) and the plane and median it names when it refuses one."""
    from imageanalysis3_amd.segmentation_tools import chromosome as CH
    rng = np.random.default_rng(12)
    d = 5e-324                                                  # the smallest float64 denormal
    for plane in ((10, 12), (9, 13)):                           # an even and an odd count
        n = plane[0] * plane[1]
        k = np.empty((5, n))
        for z in range(5):                                      # the middle value(s) are 4 d: every quotient is exact
            low, high = rng.integers(1, 4, (n - 1) // 2), rng.integers(5, 9, (n - 1) // 2)
            k[z] = rng.permutation(np.concatenate([low, [4] * (n - 2 * len(low)), high]))
        im = (k * d).reshape((5,) + plane)
        assert im.max() == 8 * d and all(np.median(p) == 4 * d for p in im)
        adj = np.array([p / np.median(p) for p in im])
        seed = ndimage.maximum_filter(adj, 3, mode='nearest') - ndimage.minimum_filter(adj, 3, mode='nearest')
        with L.ChromImage.upload(im) as dev:
            th = L.find_candidate_chromosomes(dev, 3, 90., 1, 1)[1]
        assert type(th) is np.float64 and th == scoreatpercentile(seed, 90.) and th > 0
    im = rng.random((3, 1, 4)) + 1.0
    for row, text in (([-1, -0.0, -0.0, 1], "-0"), ([-1, -0.0, 0.0, 1], "0"), ([0, np.inf, np.inf, np.inf], "inf"),
                      ([-np.inf, -np.inf, np.inf, np.inf], "-?nan")):
        bad = im.copy()
        bad[1, 0] = row
        with L.ChromImage.upload(bad) as dev:
            with pytest.raises(ValueError, match="plane 1 has the median %s:" % text):
                CH.find_candidate_chromosomes(dev, _verbose=False)
