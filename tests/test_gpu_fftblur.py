"""GPU: the box-blur normalisation kernel, the blur-normalised fft3d_from2d chain on the device and
External.Fitting_v4's twins of the FFT aligners, against tests/harness/blur_ref.py (the NumPy statement of the box
filter) and tests/golden/fftblur.npz (the reference's own results, scripts/make_fftblur_golden.py)."""
import numpy as np
import pytest

from conftest import load_golden
from harness import blur_ref

pytestmark = pytest.mark.gpu

# one axis shorter than the window, a single row, ragged tiles, several tiles both ways (tiles are 16 x 64)
BLUR_SHAPES = [(1, 40), (3, 70), (20, 107), (37, 67), (70, 300), (256, 256)]
BLUR_GBS = [2, 3, 4, 5, 9, 31]
AT_GBS = (0, 3, 4, 5, 9)
F4_GBS = (3, 4, 5)
MAX_DISP = 56


def _within_one_ulp(got, want):
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape
    assert np.all(np.isfinite(want)) and np.all(np.isfinite(got))
    return np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64))


@pytest.mark.parametrize("gb", BLUR_GBS)
@pytest.mark.parametrize("shape", BLUR_SHAPES)
def test_blurnorm2d_equals_the_numpy_statement(shape, gb):
    from imageanalysis3_amd import alignment_tools as AT
    from imageanalysis3_amd.External import Fitting_v4 as F4
    rng = np.random.RandomState(1000 * shape[0] + shape[1] + gb)
    ints = rng.randint(100, 60000, size=shape).astype(np.uint16)
    noise = rng.normal(400., 60., size=shape).astype(np.float32)
    for fn, mode in ((AT.blurnorm2d, blur_ref.DIVIDE), (F4.blurnorm2d, blur_ref.SUBTRACT)):
        # integer-valued input (any summation order is exact): bit-equal, from the uint16 array and from its float32 cast
        want = blur_ref.blurnorm2d(ints, gb, mode)
        for im in (ints, ints.astype(np.float32)):
            got = fn(im, gb)
            assert got.dtype == np.float32 and np.array_equal(got, want), (fn.__module__, shape, gb)
        # float32 noise: within one float32 ulp everywhere
        assert _within_one_ulp(fn(noise, gb), blur_ref.blurnorm2d(noise, gb, mode)), (fn.__module__, shape, gb)
    # the two modes differ only in the final operation: both are made from the one blurred image
    blurred = blur_ref.box_blur(ints.astype(np.float32), gb)
    assert np.array_equal(AT.blurnorm2d(ints, gb), ints.astype(np.float32) / blurred)
    assert np.array_equal(F4.blurnorm2d(ints, gb), ints.astype(np.float32) - blurred)


def test_blurnorm2d_reference_fixture_and_argument_errors():
    from imageanalysis3_amd import alignment_tools as AT
    from imageanalysis3_amd.External import Fitting_v4 as F4
    g = load_golden("fftblur.npz")
    for gb in (3, 4):
        assert _within_one_ulp(AT.blurnorm2d(g["blur_in"], gb), g["blur_at_gb%d" % gb])
        assert _within_one_ulp(F4.blurnorm2d(g["blur_in"], gb), g["blur_f4_gb%d" % gb])
    im = g["blur_in"]
    assert np.array_equal(AT.blurnorm2d(im, 1), np.ones_like(im))      # a 1 x 1 box is the image itself
    assert AT.blurnorm2d(im, 32).shape == im.shape                     # the largest supported box
    for fn, gb in ((AT.blurnorm2d, 0), (AT.blurnorm2d, 33), (F4.blurnorm2d, 1), (F4.blurnorm2d, 0), (F4.blurnorm2d, 33)):
        with pytest.raises(ValueError):
            fn(im, gb)
    with pytest.raises(IndexError):
        AT.blurnorm2d(np.zeros((2, 3, 4), np.float32), 3)


@pytest.fixture(scope="module")
def pairs():
    return {tag: blur_ref.bead_blob_pair(dt) for tag, dt in (("f32", np.float32), ("u16", np.uint16))}


@pytest.mark.parametrize("tag", ["f32", "u16"])
def test_fft3d_from2d_blur_chain_equals_reference(pairs, tag, monkeypatch):
    from imageanalysis3_amd import _lib as L
    from imageanalysis3_amd.alignment_tools import fft3d_from2d
    g = load_golden("fftblur.npz")
    ref, src = pairs[tag]
    # the blur decides the answer on this pair
    assert not np.array_equal(g["at_fft3d_gb0_" + tag], g["at_fft3d_gb5_" + tag])
    assert not np.array_equal(g["at_fft3d_gb3_" + tag], g["at_fft3d_gb5_" + tag])
    host = {gb: fft3d_from2d(src, ref, gb=gb, max_disp=MAX_DISP) for gb in AT_GBS}
    for gb in AT_GBS:
        assert np.array_equal(host[gb], g["at_fft3d_gb%d_%s" % (gb, tag)]), (gb, host[gb])
    with L.DeviceStack.upload(src) as ds, L.DeviceStack.upload(ref) as dr:
        def no_download(self):
            raise AssertionError("a resident stack was downloaded")
        monkeypatch.setattr(L.DeviceStack, "download", no_download)
        for gb in AT_GBS:
            got = fft3d_from2d(ds, dr, gb=gb, max_disp=MAX_DISP)
            assert got.dtype == host[gb].dtype and np.array_equal(got, host[gb]), (gb, got)


def test_fitting_v4_fftalign_2d_equals_reference():
    from imageanalysis3_amd.External.Fitting_v4 import fftalign_2d
    from imageanalysis3_amd import alignment_tools as AT
    g = load_golden("fftblur.npz")
    a, b = g["proj_src"], g["proj_ref"]
    cases = {"equal": (a, b, {}), "unequal": (a, b[:100, 10:90], {}), "centred": (a, b, dict(center=[20, -10], max_disp=8))}
    for name, (im1, im2, kw) in cases.items():
        xt, yt, cor = fftalign_2d(im1, im2, return_cor=True, **kw)
        assert np.array_equal([xt, yt], g["f4_align_" + name]), (name, xt, yt)
        assert np.isclose(cor, float(g["f4_align_cor_" + name]), rtol=1e-9, atol=0), (name, cor)
        assert np.array_equal(fftalign_2d(im1, im2, **kw), g["f4_align_" + name])
        assert np.array_equal(AT.fftalign_2d(im1, im2, **dict(dict(max_disp=50), **kw)), g["at_align_" + name])
    # the two offset conventions agree for equal shapes only
    assert np.array_equal(g["f4_align_equal"], g["at_align_equal"])
    assert not np.array_equal(g["f4_align_unequal"], g["at_align_unequal"])
    with pytest.raises(NotImplementedError):
        fftalign_2d(a, b, plt_val=True)


@pytest.mark.parametrize("tag", ["f32", "u16"])
def test_fitting_v4_fft3d_from2d_equals_reference(pairs, tag):
    from imageanalysis3_amd import _lib as L
    from imageanalysis3_amd.External.Fitting_v4 import fft3d_from2d
    g = load_golden("fftblur.npz")
    ref, src = pairs[tag]
    with L.DeviceStack.upload(src) as ds, L.DeviceStack.upload(ref) as dr:
        for gb in F4_GBS:
            for im1, im2 in ((src, ref), (ds, dr)):
                t, cor_xy, cor_z = fft3d_from2d(im1, im2, gb=gb, max_disp=MAX_DISP, return_cor=True)
                assert np.array_equal(t, g["f4_fft3d_gb%d_%s" % (gb, tag)]), (gb, t)
                want = g["f4_fft3d_cor_gb%d_%s" % (gb, tag)]
                print("gb=%d %s cor rel err" % (gb, tag), abs(cor_xy / want[0] - 1), abs(cor_z / want[1] - 1))
                assert np.allclose([cor_xy, cor_z], want, rtol=1e-9, atol=0), (gb, cor_xy, cor_z, want)
                assert np.array_equal(fft3d_from2d(im1, im2, gb=gb, max_disp=MAX_DISP), t)
    for gb in (1, 0, 33):
        with pytest.raises(ValueError):
            fft3d_from2d(src, ref, gb=gb)
    with pytest.raises(NotImplementedError):
        fft3d_from2d(src, ref, plt_val=True)


def test_align_beads_with_fft_filter():
    from imageanalysis3_amd import synth
    from imageanalysis3_amd.alignment_tools import fft3d_from2d
    from imageanalysis3_amd.correction_tools.alignment import align_beads
    g, gb = load_golden("drift.npz"), load_golden("fftblur.npz")
    ref, src, _, _ = synth.make_bead_pair(tuple(g["bead_shape"]), 120, 21, g["bead_true_d"])
    s = tuple(slice(*c) for c in g["crops_2"][0])
    rough = fft3d_from2d(src[s], ref[s], gb=5, max_disp=np.max(src[s].shape) / 2)
    assert np.array_equal(rough, gb["beads_rough_gb5"]) and np.array_equal(rough, g["pair_rough"])
    d5, t5, r5 = align_beads(g["pair_src_cts"], g["pair_ref_cts"], src[s], ref[s], fft_filt_size=5, verbose=False)
    d0, t0, r0 = align_beads(g["pair_src_cts"], g["pair_ref_cts"], src[s], ref[s], fft_filt_size=0, verbose=False)
    assert np.array_equal(d5, d0) and np.array_equal(t5, t0) and np.array_equal(r5, r0)
    assert np.allclose(d5, g["check_drift"] if "check_drift" in g else g["pair_drift"], atol=1e-12)
