"""get_seeds with the front filter's in-plane passes fused into the candidate test (seed_front_k, IA3_TUNE_SEED_FUSED = 1)
against the two-kernel path (plane-wise filter into a stack + tiled detector, IA3_TUNE_SEED_FUSED = 0): identical tables
(coordinates, heights, order) on the bench FOV, crowded fields, ragged shapes at every folded depth, spots on the border
planes, rows and columns and on both sides of the z-chunk boundary, both edge distances, uint16 plateaus, mixed-sign
float32, row lengths with and without the column kernel's strip minima, and the lazy path's overflow fallback."""
import ctypes as C
import numpy as np
import pytest
from imageanalysis3_amd._lib import IA3_TUNE_SEED_FUSED, IA3_TUNE_SEED_DENSE

pytestmark = pytest.mark.gpu


def _tune(key, value):
    from imageanalysis3_amd import _lib as L
    L.check(L.lib().ia3_set_tuning(C.c_int(key), C.c_int(value)))


def _both(im, **kw):
    from imageanalysis3_amd.spot_tools.fitting import get_seeds
    try:
        _tune(IA3_TUNE_SEED_FUSED, 0)
        old = get_seeds(im, return_h=True, **kw)
        _tune(IA3_TUNE_SEED_FUSED, 1)
        new = get_seeds(im, return_h=True, **kw)
    finally:
        _tune(IA3_TUNE_SEED_FUSED, 1)
    return old, new


def _same(im, **kw):
    old, new = _both(im, **kw)
    assert old.shape == new.shape and np.array_equal(old, new), (im.shape, im.dtype, old.shape, new.shape)
    return new


@pytest.mark.parametrize("dtype", [np.float32, np.uint16])
def test_fused_bench_fov(dtype):
    from imageanalysis3_amd import synth
    im, c, h = synth.make_fov((50, 2048, 2048), 5000, 1, dtype=dtype)
    s = _same(im, th_seed=600.0)
    assert len(s) > 1000


def test_fused_crowded_field():
    from imageanalysis3_amd import synth
    im, c, h = synth.make_fov((50, 1024, 1024), 6000, 7, layout="clustered")
    s = _same(im, th_seed=600.0)
    assert len(s) > 500


def _borders(im, zc, val):
    """bright voxels on the first / last plane, row and column and on either side of the z-chunk boundary"""
    Z, X, Y = im.shape
    for z, x, y in ((0, X // 2, Y // 3), (Z - 1, X // 3, Y // 2), (Z // 2, 0, Y // 4), (Z // 3, X - 1, Y // 5),
                    (Z // 4, X // 5, 0), (Z // 5 + 1, X // 4, Y - 1), (zc - 1, X // 2, Y // 2), (zc, X // 2 + 5, Y // 2 + 9),
                    (0, 0, 0), (Z - 1, X - 1, Y - 1), (zc, 15, 127), (zc - 1, 16, 128)):
        im[z, min(x, X - 1), min(y, Y - 1)] += val
    return im


@pytest.mark.parametrize("shape,dtype", [((25, 70, 300), np.float32), ((30, 33, 257), np.uint16), ((40, 130, 70), np.float32),
                                         ((50, 75, 200), np.uint16), ((60, 47, 390), np.float32), ((50, 200, 256), np.float32),
                                         ((30, 100, 96), np.uint16), ((40, 17, 130), np.uint16)])
@pytest.mark.parametrize("edge", [0, 2])
def test_fused_ragged_shapes_and_borders(shape, dtype, edge):
    from imageanalysis3_amd import synth
    im, c, h = synth.make_fov(shape, 20, 31, dtype=dtype, margin=(2, 6, 6), layout="uniform")
    im = _borders(im, (shape[0] + 1) // 2, 3000)
    s = _same(im, th_seed=300.0, min_edge_distance=edge)
    if edge == 0:
        Z, X, Y = shape
        zxy = s[:, :3].astype(int)
        assert ((zxy[:, 0] == 0) | (zxy[:, 0] == Z - 1) | (zxy[:, 1] == 0) | (zxy[:, 1] == X - 1)
                | (zxy[:, 2] == 0) | (zxy[:, 2] == Y - 1)).any()


def test_fused_u16_plateaus():
    steps = (np.arange(50 * 96 * 200).reshape(50, 96, 200) // 517 % 7 * 500 + 300).astype(np.uint16)
    steps[20:23, 40:43, 150:153] += 2000
    steps[24:26, 10:12, 0:2] += 1500        # a plateau across the z-chunk boundary, on the first columns
    _same(steps, th_seed=200.0)
    steps32 = (np.arange(50 * 96 * 192).reshape(50, 96, 192) // 517 % 7 * 500 + 300).astype(np.uint16)
    steps32[20:23, 40:43, 150:153] += 2000
    steps32[40:, :, :96] += 150
    _same(steps32, th_seed=200.0)


def test_fused_mixed_sign_f32():
    rng = np.random.default_rng(5)
    for shape in ((50, 90, 210), (50, 90, 224)):
        mixed = rng.normal(0, 50, size=shape).astype(np.float32)
        mixed[8:11, 30:33, 60:63] += 900
        mixed[30:33, 70:73, 190:193] += 700
        mixed[5, 70, 20] = -4000.0
        mixed[25:, 40:, :] += 120.0
        _same(mixed, th_seed=150.0)


def test_fused_overflow_falls_back_to_dense():
    from imageanalysis3_amd.spot_tools.fitting import get_seeds
    rng = np.random.default_rng(3)
    noise = rng.normal(400, 60, size=(30, 512, 512)).astype(np.float32)
    kw = dict(th_seed=5.0, use_dynamic_th=False, remove_hot_pixel=False)
    new = _same(noise, **kw)
    try:
        _tune(IA3_TUNE_SEED_DENSE, 1)
        dense = get_seeds(noise, return_h=True, **kw)
    finally:
        _tune(IA3_TUNE_SEED_DENSE, 0)
    assert np.array_equal(dense, new)
