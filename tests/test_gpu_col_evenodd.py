"""The column kernel's even/odd long pass and the short pass on the recovered column (csrc/gauss_col_kernel.inc) on
inputs built for its rules: mirror pairs of outputs that differ by orders of magnitude (rule (i): both take the reference
sequence), float32 columns whose mirror planes do not add up exactly (the short pass comes from memory, for the whole
wave), sign bits, sums on quantisation boundaries, zeros.  Built depths only (50 even, 33 odd), one wave per row of a
(Z, 16, 64) stack, bit for bit against SciPy with the guard at its default, off and wide open."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CERTS = (-2, -1, 1 << 28)
DEPTHS = (50, 33)


def _set_gauss_cert(v):
    from imageanalysis3_amd import _lib as L
    L.check(L.lib().ia3_set_tuning(L.IA3_TUNE_GAUSS_CERT, C.c_int(v)))


@functools.lru_cache(maxsize=None)
def _stack(Z, dtype):
    """(Z, 16, 64): row x is one wave of the kernel; the rows hold the cases of the module's docstring."""
    rng = np.random.RandomState(100 + Z + (0 if dtype == "float32" else 1))
    shape = (Z, 16, 64)
    H = Z // 2
    if dtype == "float32":
        im = rng.gamma(2.0, 300.0, size=shape).astype(np.float32)
        half = np.zeros((Z, 2, 64), np.float32)
        half[H + 3:] = rng.uniform(0.0, 6e4, size=(Z - H - 3, 2, 64))
        im[:, 0:2] = half                                  # zero in one half, up to 6e4 in the other
        im[:, 2:4] = half[::-1]                            # and its mirror
        im[:H, 4] = 1e-20                                  # mirror planes a hundred binades apart: E and O are not exact
        im[Z - H:, 4] = 1e10
        im[H - 2:H + 3, 5, ::4] = 1e-20                    # the small value in the centre planes of every fourth column
        im[3:6, 6, 10:30] = -0.0                           # sign bit without a negative value
        im[7, 7, ::3] = -250.0                             # a negative value
        im[:, 8] = 0.0                                     # a wave of zero columns
        im[:, 9, :32] = 0.0                                # and half a wave
    else:
        im = np.clip(rng.gamma(2.0, 300.0, size=shape), 0, 65535).astype(np.uint16)
        im[0::2, 0:2] = 0                                  # planes alternating 0 / 65535
        im[1::2, 0:2] = 65535
        for x in (2, 3, 4, 5):                             # piecewise constant with a step along z: sums on integer boundaries
            for y0 in range(0, 64, 16):
                v = int(rng.randint(1, 65535))
                im[:, x, y0:y0 + 16] = v
                im[int(rng.randint(0, Z)):, x, y0:y0 + 16] = v // 3
        im[:, 6] = 0                                       # zero columns
        im[:H + 3, 7:9] = 0                                # zero in one half
        im[:, 9:11] = im[::-1, 7:9]                        # and its mirror
        im[H + 3:, 7] = 60000
    im.setflags(write=False)
    return im


@functools.lru_cache(maxsize=None)
def _refs(Z, dtype):
    from scipy import ndimage as ndi
    im = _stack(Z, dtype)
    out = {"front": ndi.gaussian_filter(im, 0.75, mode="reflect", truncate=4.0),
           "back": ndi.gaussian_filter1d(im, 7.5, axis=0, mode="reflect", truncate=4.0)}
    for mode in ("reflect", "nearest"):
        out[mode] = ndi.gaussian_filter(im, 7.5, mode=mode, truncate=4.0)
    return out


def _bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint16)


def _where(got, ref):
    bad = np.argwhere(_bits(got) != _bits(ref))
    return len(bad), bad[:4].tolist()


@pytest.mark.parametrize("dtype", ["float32", "uint16"])
@pytest.mark.parametrize("Z", DEPTHS)
def test_dog_filter_pair_on_evenodd_edge_inputs(Z, dtype):
    """ia3_dog_filters_dev: both outputs of the pair launch, the short pass from the recovered column or from memory."""
    from imageanalysis3_amd import _lib as L
    lib = L.lib()
    assert lib.ia3_prepare_depth(L.dtype_code(np.zeros(1, dtype)), Z) == 1
    im, ref = _stack(Z, dtype), _refs(Z, dtype)
    try:
        for cert in CERTS:
            _set_gauss_cert(cert)
            with L.DeviceStack.upload(np.array(im)) as st, L.DeviceStack.empty(im.shape, im.dtype) as f, \
                    L.DeviceStack.empty(im.shape, im.dtype) as b:
                L.check(lib.ia3_dog_filters_dev(st._h, C.c_double(0.75), C.c_double(7.5), f._h, b._h))
                got_f, got_b = f.download(), b.download()
            assert np.array_equal(_bits(got_b), _bits(ref["back"])), (Z, dtype, cert, "back") + _where(got_b, ref["back"])
            assert np.array_equal(_bits(got_f), _bits(ref["front"])), (Z, dtype, cert, "front") + _where(got_f, ref["front"])
    finally:
        _set_gauss_cert(-2)


@pytest.mark.parametrize("mode", ["reflect", "nearest"])
@pytest.mark.parametrize("dtype", ["float32", "uint16"])
@pytest.mark.parametrize("Z", DEPTHS)
def test_single_long_pass_on_evenodd_edge_inputs(Z, dtype, mode):
    """correction_tools.filter.gaussian_filter: the axis-0 pass alone in the column kernel (RF = 0), both border modes."""
    from imageanalysis3_amd.correction_tools.filter import gaussian_filter
    im, ref = _stack(Z, dtype), _refs(Z, dtype)[mode]
    try:
        for cert in CERTS:
            _set_gauss_cert(cert)
            got = gaussian_filter(np.array(im), 7.5, mode=mode, truncate=4.0)
            assert np.array_equal(_bits(got), _bits(ref)), (Z, dtype, mode, cert) + _where(got, ref)
    finally:
        _set_gauss_cert(-2)


@pytest.mark.parametrize("case", ["float32", "uint16", "float32_inexact_pairs"])
def test_seeds_equal_the_oracle(case):
    """ia3_dog_seed on a (50, 64, 128) field: the pair launch with its strip minima and maxima feeding the detector.  The
    third case plants tiny values, so that some waves take their short pass (and its strip maxima) from memory."""
    if os.path.join(ROOT, "oracle") not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import np_oracle as O
    from imageanalysis3_amd import synth
    from imageanalysis3_amd.spot_tools.fitting import get_seeds
    dtype = np.uint16 if case == "uint16" else np.float32
    im = synth.make_fov((50, 64, 128), 40, 5, dtype=dtype)[0]
    if case == "float32_inexact_pairs":
        im = im.copy()
        im[20:30, ::7, ::5] = 1e-20
        im[0, 3::11, 2::9] = 1e-25
    seeds = get_seeds(im, th_seed=600, return_h=True)
    ref = O.get_seeds(im, th_seed=600, return_h=True)
    assert len(ref) >= 10 and seeds.shape == ref.shape, (case, seeds.shape, ref.shape)
    # rows sorted by coordinate: seeds of equal height (uint16) may come in either order
    got_s, ref_s = (s[np.lexsort((s[:, 2], s[:, 1], s[:, 0]))] for s in (np.asarray(seeds), np.asarray(ref)))
    assert np.array_equal(got_s, ref_s), (case, got_s[(got_s != ref_s).any(axis=1)].tolist(), ref_s[(got_s != ref_s).any(axis=1)].tolist())
