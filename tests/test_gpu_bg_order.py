"""get_seeds with the sparse background pass testing the centre plane first (IA3_TUNE_SEED_BGORDER = 1, the default: the
planes z - 1 and z + 1 only for candidates whose answer needs them) against the same kernels evaluating all 27 values for
every candidate (0), against the dense background filter and against the oracle: identical tables (coordinates, heights,
order), and the counter of ia3_seed_bg_stats shows which candidates took the outer planes.  The fixture holds a candidate
of every class: accepted in-plane (interior: the 63-row path; near the x border: the row-by-row path), accepted only
through a neighbouring plane, rejected after all 27 values."""
import ctypes as C
import numpy as np
import pytest

import np_oracle as O
from imageanalysis3_amd._lib import IA3_TUNE_SEED_BGORDER, IA3_TUNE_SEED_DENSE, IA3_TUNE_COL_RTC

pytestmark = pytest.mark.gpu

SHAPE = (25, 96, 128)   # a paired column-kernel depth; rows of 128: strip bound; X = 96: interior and border candidates
SPOTS = [(8, 40, 40), (12, 48, 96), (17, 70, 30), (10, 6, 70)]
TH = 600.0


def _tune(key, value):
    from imageanalysis3_amd import _lib as L
    L.check(L.lib().ia3_set_tuning(C.c_int(key), C.c_int(value)))


def _bg_stats():
    """(candidates tested by the sparse pass, those that took the outer planes) of this thread's last get_seeds"""
    from imageanalysis3_amd import _lib as L
    out = (C.c_double * 2)()
    L.check(L.lib().ia3_seed_bg_stats(out))
    return int(out[0]), int(out[1])


def _units():
    from imageanalysis3_amd import _lib as L
    out = (C.c_double * 2)()
    L.check(L.lib().ia3_seed_skip_stats(out))
    return out[0], out[1]


def make_fixture(dtype, shape=SHAPE, spots=SPOTS):
    """A flat background of 400 with two patches and spots of height 3000 (sigma 1).  Around spots[0]: a clipped
    paraboloid bowl in (x, y), 2 per squared pixel, radius 11, over 13 planes with a ramp of 6 per plane in z: min_im has
    its in-plane minimum at the spot and falls towards z - 1.  Around spots[1]: a 3-D bowl: a true 3 x 3 x 3 minimum."""
    Z, X, Y = shape
    z, x, y = np.meshgrid(np.arange(Z), np.arange(X), np.arange(Y), indexing="ij")
    im = np.full(shape, 400.0)
    z0, x0, y0 = spots[0]
    d2 = (x - x0) ** 2 + (y - y0) ** 2
    patch = (d2 < 121) & (abs(z - z0) <= 6)
    im[patch] = (400.0 - 2.0 * (121 - d2) + 6.0 * (z - z0))[patch]
    z1, x1, y1 = spots[1]
    im -= np.clip(240.0 - (2.0 * ((x - x1) ** 2 + (y - y1) ** 2) + 8.0 * (z - z1) ** 2), 0, None)
    for sz, sx, sy in spots:
        im += 3000.0 * np.exp(-((z - sz) ** 2 + (x - sx) ** 2 + (y - sy) ** 2) / 2.0)
    assert im.min() >= 0
    return im.astype(np.float32) if np.dtype(dtype) == np.float32 else np.floor(im).astype(np.uint16)


def oracle_classes(im, th, edge=2):
    """{(z, x, y): 'inplane' | 'outer' | 'reject'} of the first-stage candidates (local maxima of max_im with
    diff >= th inside the edge margin), from the oracle's min_im"""
    max_im = O.gaussian_filter(im, 0.75)
    min_im = O.gaussian_filter(im, 7.5)
    diff = max_im.astype(np.float32) - min_im.astype(np.float32)
    c = np.array(np.where((O.maximum_filter3(max_im) == max_im) & (diff >= th))).T
    size = np.array(im.shape)
    if edge > 0:
        c = c[((c >= edge) & (c <= size - edge)).all(1)]
    out = {}
    for zc, xc, yc in c:
        idx = [[min(max(v + d, 0), n - 1) for d in (-1, 0, 1)] for v, n in zip((zc, xc, yc), im.shape)]
        nb = min_im[np.ix_(*idx)]
        cm = min_im[zc, xc, yc]
        out[(int(zc), int(xc), int(yc))] = ("inplane" if (nb[1] < cm).any() else
                                            "outer" if ((nb[0] < cm).any() or (nb[2] < cm).any()) else "reject")
    return out


def _three(im, **kw):
    """tables with the key at 1, at 0 and from the dense filter, and the counters of the two sparse runs"""
    from imageanalysis3_amd.spot_tools.fitting import get_seeds
    try:
        _tune(IA3_TUNE_SEED_BGORDER, 1)
        new = get_seeds(im, return_h=True, **kw)
        st_new = _bg_stats()
        _three.units = _units()                          # (tile, plane) units of the fused detector in the key-1 run
        _tune(IA3_TUNE_SEED_BGORDER, 0)
        old = get_seeds(im, return_h=True, **kw)
        st_old = _bg_stats()
        _tune(IA3_TUNE_SEED_BGORDER, 1)
        _tune(IA3_TUNE_SEED_DENSE, 1)
        dense = get_seeds(im, return_h=True, **kw)
        st_dense = _bg_stats()
    finally:
        _tune(IA3_TUNE_SEED_BGORDER, 1)
        _tune(IA3_TUNE_SEED_DENSE, 0)
    print("sparse pass, tested / outer planes: key 1 %d / %d, key 0 %d / %d" % (st_new + st_old), im.shape, im.dtype)
    assert new.shape == old.shape and np.array_equal(new, old, equal_nan=True), (new, old)
    assert new.shape == dense.shape and np.array_equal(new, dense, equal_nan=True), (new, dense)
    assert st_old[0] == st_old[1] and st_new[0] == st_old[0] and st_new[1] <= st_new[0]   # key 0: every candidate takes all planes
    assert st_dense == (0, 0)
    return new, st_new, st_old


_fixtures = {}


@pytest.fixture(params=[np.float32, np.uint16], ids=["f32", "u16"])
def fixture_and_oracle(request):
    """(image, oracle seeds, oracle classes), computed once per dtype and left unchanged"""
    key = np.dtype(request.param).name
    if key not in _fixtures:
        im = make_fixture(request.param)
        im.setflags(write=False)
        _fixtures[key] = (im, O.get_seeds(im, th_seed=TH, return_h=True), oracle_classes(im, TH))
    return _fixtures[key]


def test_fixture_holds_every_class(fixture_and_oracle):
    im, ref, cls = fixture_and_oracle
    assert cls[SPOTS[0]] == "outer" and cls[SPOTS[1]] == "reject" and cls[SPOTS[2]] == "inplane" and cls[SPOTS[3]] == "inplane", cls
    for k in (0, 1):                                     # the 63-row path: the outer planes are taken through it
        assert SPOTS[k][1] - 31 >= 0 and SPOTS[k][1] + 31 < im.shape[1]
    assert SPOTS[3][1] - 31 < 0 and SPOTS[2][1] + 31 >= im.shape[1]   # the row-by-row path on either x border
    assert {tuple(int(v) for v in r[:3]) for r in ref} == {SPOTS[0], SPOTS[2], SPOTS[3]}       # 3 seeds of the 4 spots


def test_fixture_key1_key0_dense_oracle(fixture_and_oracle):
    im, ref, cls = fixture_and_oracle
    assert cls[SPOTS[0]] == "outer" and cls[SPOTS[1]] == "reject" and "inplane" in cls.values(), cls   # the input's condition
    new, st_new, st_old = _three(im, th_seed=TH)
    assert new.shape == ref.shape and np.array_equal(new, ref), (new, ref)
    assert st_new[1] >= 2 and st_new[1] < st_new[0]
    assert _three.units[1] > 0                          # depth 25: the paired column kernel and the fused detector


def _rows_sorted(t):
    return t[np.lexsort(t.T[::-1])] if len(t) else t


@pytest.mark.parametrize("dtype", [np.float32, np.uint16])
def test_borders(dtype):
    Z, X, Y = SHAPE
    spots = [(0, 40, 40), (Z - 1, 48, 96), (17, 0, 30), (10, 50, 0), (12, 70, Y - 1), (Z - 1, X - 1, 60), (0, 20, 100)]
    im = make_fixture(dtype, spots=spots)
    new, st_new, st_old = _three(im, th_seed=TH, min_edge_distance=0)
    ref = O.get_seeds(im, th_seed=TH, return_h=True, min_edge_distance=0)
    assert new.shape == ref.shape and np.array_equal(_rows_sorted(new), _rows_sorted(ref)), (new, ref)   # (equal heights)
    assert st_new[0] >= len(spots) and st_new[1] >= 1   # the bowl on plane 0: z - 1 clamps onto z
    zxy = new[:, :3].astype(int)
    assert (zxy[:, 0] == 0).any() or (zxy[:, 0] == Z - 1).any() or (zxy[:, 1] == 0).any() or (zxy[:, 2] == 0).any() \
        or (zxy[:, 2] == Y - 1).any()


@pytest.mark.parametrize("dtype", [np.float32, np.uint16])
def test_unfused_path(dtype):
    """a depth without a built-in column kernel, with its run-time compilation off: sliding-window axis-0 passes, the
    plane-wise front filter, the tiled candidate kernel and the sparse pass of launch_lazy's stage 1"""
    spots = [(4, 40, 40), (6, 48, 96), (8, 70, 30), (5, 6, 70)]
    im = make_fixture(dtype, shape=(12, 96, 128), spots=spots)
    try:
        _tune(IA3_TUNE_COL_RTC, 0)
        new, st_new, st_old = _three(im, th_seed=TH)
        u = _three.units
    finally:
        _tune(IA3_TUNE_COL_RTC, 1)
    assert u == (0.0, 0.0) and st_new[0] >= len(spots)   # no fused detector, and the sparse pass ran
    ref = O.get_seeds(im, th_seed=TH, return_h=True)
    assert new.shape == ref.shape and np.array_equal(new, ref), (new, ref)
    assert len(new) >= 2


@pytest.mark.parametrize("dtype", [np.float32, np.uint16])
def test_generic_radius(dtype):
    """background_gfilt_size = 5: radius 20, the any-radius kernel.  (One threshold level: on the unfused path the list is
    made at the lowest level, and with ten levels the flat voxels of the blocks that hold a bowl would fill it up and send
    the stage to the dense filter.)"""
    im = make_fixture(dtype)
    kw = dict(th_seed=TH, background_gfilt_size=5, use_dynamic_th=False)
    new, st_new, st_old = _three(im, **kw)
    ref = O.get_seeds(im, return_h=True, **kw)
    assert new.shape == ref.shape and np.array_equal(_rows_sorted(new), _rows_sorted(ref)), (new, ref)   # (equal heights: NumPy's order is its own)
    assert st_new[0] >= 4 and len(new) >= 2


def test_u16_plateau():
    """a constant uint16 background: the truncated min_im is one plateau, all 27 values are equal, every candidate takes
    the outer planes and is rejected; at every level the dynamic threshold visits"""
    from imageanalysis3_amd.spot_tools.fitting import get_seeds
    im = np.full(SHAPE, 400, np.uint16)
    for z, x, y in SPOTS + [(0, 50, 50), (24, 3, 3)]:
        im[z, x, y] += 3000
    new, st_new, st_old = _three(im, th_seed=TH, min_edge_distance=0)
    ref = O.get_seeds(im, th_seed=TH, return_h=True, min_edge_distance=0)
    assert new.shape == ref.shape and np.array_equal(new, ref), (new, ref)
    assert st_new[0] >= 6 and st_new[1] >= 6
    for it in range(10):                                 # the levels of the dynamic threshold, one by one
        th = TH * (1 - it / 10)
        kw = dict(th_seed=th, use_dynamic_th=False, min_edge_distance=0, return_h=True)
        dev = []
        try:
            for v in (1, 0):
                _tune(IA3_TUNE_SEED_BGORDER, v)
                dev.append(get_seeds(im, **kw))
        finally:
            _tune(IA3_TUNE_SEED_BGORDER, 1)
        ref = O.get_seeds(im, **kw)
        assert dev[0].shape == ref.shape and np.array_equal(dev[0], ref) and np.array_equal(dev[1], ref), (th, dev, ref)


def test_u16_ties():
    from imageanalysis3_amd import synth
    im, c, h = synth.make_fov((25, 160, 192), 60, 5, dtype=np.uint16)
    new, st_new, st_old = _three(im, th_seed=TH)
    print("uint16 ties: %d of %d candidates took the outer planes, %d seeds" % (st_new[1], st_new[0], len(new)))
    assert len(new) > 20 and st_new[0] >= len(new)
