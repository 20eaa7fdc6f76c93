"""get_seeds with the fused detector skipping the planes of a tile that cannot hold a candidate (IA3_TUNE_SEED_SKIP = 1)
and with the first-stage list made at the first dynamic level as well (2, the default) against the same detector running
every plane with the list at the lowest level (0): identical tables (coordinates, heights, order), and the
counter of (tile, plane) units shows that planes really were left out, on the bench FOV in both dtypes, a crowded field,
ragged shapes with spots on the border planes, rows and columns, on both sides of the z-chunk boundary, next to a gap of
dead planes and in the halo of a dead neighbouring tile, uint16 plateaus, mixed-sign float32 with negative strip maxima,
NaN and +inf next to a spot, a noise-only stack under the dynamic threshold (against the dense filter) and a row length
without strip outputs (nothing skipped)."""
import ctypes as C
import numpy as np
import pytest
from imageanalysis3_amd._lib import IA3_TUNE_SEED_SKIP, IA3_TUNE_SEED_DENSE

pytestmark = pytest.mark.gpu


def _tune(key, value):
    from imageanalysis3_amd import _lib as L
    L.check(L.lib().ia3_set_tuning(C.c_int(key), C.c_int(value)))


def _units():
    """(units run, units in all) of this thread's last get_seeds"""
    from imageanalysis3_amd import _lib as L
    out = (C.c_double * 2)()
    L.check(L.lib().ia3_seed_skip_stats(out))
    return out[0], out[1]


def _all(im, **kw):
    """tables and unit counts with the key at 0 (every plane, list at the lowest level), 1 (skipping) and 2 (skipping and
    the list at the first dynamic level, the default)"""
    from imageanalysis3_amd.spot_tools.fitting import get_seeds
    res = []
    try:
        for v in (0, 1, 2):
            _tune(IA3_TUNE_SEED_SKIP, v)
            res.append((get_seeds(im, return_h=True, **kw), _units()))
    finally:
        _tune(IA3_TUNE_SEED_SKIP, 2)
    return res


def _same(im, **kw):
    (old, u_old), (new, u_new), (top, u_top) = _all(im, **kw)
    print("units run / all: key 0 %d / %d, key 1 %d / %d, key 2 %d / %d" % (u_old + u_new + u_top), im.shape, im.dtype)
    assert old.shape == new.shape and np.array_equal(old, new, equal_nan=True), (im.shape, im.dtype, old.shape, new.shape)
    assert old.shape == top.shape and np.array_equal(old, top, equal_nan=True), (im.shape, im.dtype, old.shape, top.shape)
    assert u_old[0] == u_old[1]                      # key at 0: every unit runs (0 == 0 where the fused detector does not run)
    assert u_new[1] == u_old[1] and u_new[0] <= u_new[1]
    assert u_top[1] == u_old[1] and u_top[0] <= u_top[1]
    return new, u_new


@pytest.mark.parametrize("dtype", [np.float32, np.uint16])
def test_skip_bench_fov(dtype):
    from imageanalysis3_amd import synth
    im, c, h = synth.make_fov((50, 2048, 2048), 5000, 1, dtype=dtype)
    s, u = _same(im, th_seed=600.0)
    assert len(s) > 1000
    assert u[1] > 0 and u[0] < u[1]                  # the path under test is the skipping one


def test_skip_crowded_field():
    from imageanalysis3_amd import synth
    im, c, h = synth.make_fov((50, 1024, 1024), 6000, 7, layout="clustered")
    s, u = _same(im, th_seed=600.0)
    assert len(s) > 500 and u[1] > 0


def _borders(im, zc, val):
    """bright voxels on the first / last plane, row and column, on either side of the z-chunk boundary, and on the last
    rows / columns of one detector tile and the first of the next (16 x 128 tiles)"""
    Z, X, Y = im.shape
    for z, x, y in ((0, X // 2, Y // 3), (Z - 1, X // 3, Y // 2), (Z // 2, 0, Y // 4), (Z // 3, X - 1, Y // 5),
                    (Z // 4, X // 5, 0), (Z // 5 + 1, X // 4, Y - 1), (zc - 1, X // 2, Y // 2), (zc, X // 2 + 5, Y // 2 + 9),
                    (0, 0, 0), (Z - 1, X - 1, Y - 1), (zc, 15, 127), (zc - 1, 16, 128), (zc + 3, 31, 31), (zc - 4, 32, 32)):
        im[z, min(x, X - 1), min(y, Y - 1)] += val
    return im


@pytest.mark.parametrize("shape,dtype", [((25, 70, 288), np.float32), ((30, 33, 256), np.uint16), ((40, 130, 64), np.float32),
                                         ((50, 75, 192), np.uint16), ((60, 47, 384), np.float32), ((50, 200, 256), np.float32),
                                         ((30, 100, 96), np.uint16), ((40, 17, 128), np.uint16)])
@pytest.mark.parametrize("edge", [0, 2])
def test_skip_ragged_shapes_and_borders(shape, dtype, edge):
    from imageanalysis3_amd import synth
    im, c, h = synth.make_fov(shape, 20, 31, dtype=dtype, margin=(2, 6, 6), layout="uniform")
    im = _borders(im, (shape[0] + 1) // 2, 3000)
    s, u = _same(im, th_seed=300.0, min_edge_distance=edge)
    assert u[1] > 0
    if edge == 0:
        Z, X, Y = shape
        zxy = s[:, :3].astype(int)
        assert ((zxy[:, 0] == 0) | (zxy[:, 0] == Z - 1) | (zxy[:, 1] == 0) | (zxy[:, 1] == X - 1)
                | (zxy[:, 2] == 0) | (zxy[:, 2] == Y - 1)).any()


@pytest.mark.parametrize("dtype", [np.float32, np.uint16])
def test_skip_lone_spots_between_dead_planes(dtype):
    """a flat stack (every plane dead) with single voxels: each is the only live plane of its tile, with a gap on both
    sides; on the first and last plane of a chunk; one in the corner of a tile whose own planes are dead while the
    neighbouring tiles see it in their halo; two live planes one dead plane apart"""
    Z, X, Y = 50, 96, 384
    im = np.full((Z, X, Y), 500, dtype)
    zc = (Z + 1) // 2
    pts = [(10, 40, 200), (zc - 1, 8, 8), (zc, 70, 300), (0, 50, 50), (Z - 1, 60, 350), (12, 15, 127), (30, 16, 128),
           (20, 31, 255), (22, 31, 255), (40, 0, 0), (41, X - 1, Y - 1), (5, 47, 129), (7, 48, 126)]
    for z, x, y in pts:
        im[z, x, y] += 4000
    s, u = _same(im, th_seed=300.0, min_edge_distance=0)
    assert u[0] < u[1]
    if dtype == np.float32:   # (on a flat uint16 stack the truncated background is a plateau around a spot: the reference's own rule drops it)
        found = {tuple(r) for r in s[:, :3].astype(int)}
        assert set(pts) <= found, set(pts) - found


def test_skip_u16_plateaus():
    steps32 = (np.arange(50 * 96 * 192).reshape(50, 96, 192) // 517 % 7 * 500 + 300).astype(np.uint16)
    steps32[20:23, 40:43, 150:153] += 2000
    steps32[24:26, 10:12, 0:2] += 1500        # a plateau across the z-chunk boundary, on the first columns
    steps32[40:, :, :96] += 150
    _same(steps32, th_seed=200.0)
    flat = np.full((50, 96, 192), 300, np.uint16)
    flat[20:23, 40:43, 150:153] += 2000       # a plateau in a dead surrounding
    flat[24:26, 10:12, 0:2] += 1500
    s, u = _same(flat, th_seed=200.0)
    assert u[0] < u[1]


def test_skip_mixed_sign_f32():
    rng = np.random.default_rng(5)
    mixed = rng.normal(0, 50, size=(50, 90, 224)).astype(np.float32)
    mixed[8:11, 30:33, 60:63] += 900
    mixed[30:33, 70:73, 190:193] += 700
    mixed[5, 70, 20] = -4000.0
    mixed[25:, 40:, :] += 120.0
    _same(mixed, th_seed=150.0)
    neg = (-np.abs(rng.normal(0, 5, size=(50, 90, 224))) - 1000.0).astype(np.float32)   # every strip maximum is negative
    neg[8:11, 30:33, 60:63] += 900
    neg[30, 70, 190] += 2500                                                              # up to a positive value
    _same(neg, th_seed=150.0)


def test_skip_nan_and_inf_next_to_a_spot():
    rng = np.random.default_rng(6)
    for bad in (np.nan, np.inf):
        im = (rng.normal(400, 5, size=(50, 96, 256))).astype(np.float32)
        im[10, 40, 100] += 3000
        im[10, 42, 103] = bad
        im[30, 20, 200] += 3000
        im[36, 70, 30] = bad
        _same(im, th_seed=300.0, min_edge_distance=0)


def test_skip_noise_only_dynamic_threshold_against_dense():
    from imageanalysis3_amd.spot_tools.fitting import get_seeds
    rng = np.random.default_rng(8)
    noise = rng.normal(400, 12, size=(30, 256, 256)).astype(np.float32)
    kw = dict(th_seed=600.0, use_dynamic_th=True, remove_hot_pixel=False)
    new, u = _same(noise, **kw)
    try:
        _tune(IA3_TUNE_SEED_DENSE, 1)
        dense = get_seeds(noise, return_h=True, **kw)
    finally:
        _tune(IA3_TUNE_SEED_DENSE, 0)
    assert np.array_equal(dense, new)


def test_skip_row_length_without_strips():
    from imageanalysis3_amd import synth
    im, c, h = synth.make_fov((50, 75, 200), 20, 31, margin=(2, 6, 6), layout="uniform")   # Y % 32 != 0
    s, u = _same(im, th_seed=300.0)
    assert u[0] == u[1] and u[1] > 0          # no strip outputs: nothing skipped
