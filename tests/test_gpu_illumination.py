"""GPU: exact order statistics and percentiles of a resident stack, the clip-and-sum over z, the float64 2-D Gaussian and
the illumination-profile generator built on them (csrc/stats.hip, correction_tools/illumination.py).

Every comparison is bit-exact: each step is integer selection or float64 arithmetic in a fixed order.  References:
np.sort, spot_tools.fitting._score_at_percentile (pinned to SciPy by test_host_logic_cpu.py), tests/harness/illum_ref.py
(pinned to the reference by test_illumination_cpu.py), np_oracle.correlate1d and tests/golden/illum.npz (the
reference's own outputs)."""
import os

import numpy as np
import pytest

from conftest import build_case, load_golden
from harness import illum_ref

pytestmark = pytest.mark.gpu

# 105 voxels (no multiple of a vector or a block), an odd middle size, several blocks
STAT_SHAPES = [(3, 5, 7), (7, 33, 17), (12, 64, 96)]
DTYPES = [np.uint16, np.float32]


def _ranks(n):
    return [0, 1, n // 2 - 1, n // 2, n - 2, n - 1, n // 2]   # the last one repeats a rank


def _contents(shape, dtype):
    """name -> stack: the value patterns the select has to get right."""
    n = int(np.prod(shape))
    rng = np.random.RandomState(n + (0 if dtype == np.uint16 else 1))
    d = {}
    noise = rng.normal(400., 35., size=shape)
    d["noise"] = np.clip(noise, 0, 65535).astype(np.uint16) if dtype == np.uint16 else (noise - 390.).astype(np.float32)
    d["constant"] = np.full(shape, 777, dtype=dtype)
    two = np.full(n, 300, dtype=dtype)
    two[n // 2:] = 4000                       # ranks n//2 - 1 and n//2 fall on either side of the step
    d["two_valued"] = rng.permutation(two).reshape(shape)
    if dtype == np.uint16:
        ext = rng.randint(0, 65536, size=n).astype(np.uint16)
        ext[:4] = (0, 0, 65535, 65535)
        d["extremes"] = rng.permutation(ext).reshape(shape)
        d["same_high_byte"] = (0x1200 + rng.randint(0, 256, size=shape)).astype(np.uint16)
    else:
        sp = rng.normal(0., 50., size=n).astype(np.float32)
        sp[:10] = (0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 1e-40, -1e-40, -3.5, 3.5)
        d["signs_inf_denormals"] = rng.permutation(sp).reshape(shape)
        d["zeros_and_denormals"] = rng.permutation(np.resize(np.array([0.0, -0.0, 1e-45, -1e-45, 3e-39, -3e-39],
                                                                      np.float32), n)).reshape(shape)
    return d


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", STAT_SHAPES)
def test_order_statistics_equal_sorted_ranks(shape, dtype):
    from imageanalysis3_amd import _lib as L
    n = int(np.prod(shape))
    for name, im in _contents(shape, dtype).items():
        want = np.sort(im, axis=None)[_ranks(n)]
        with L.DeviceStack.upload(im) as st:
            got = st.order_stats(_ranks(n))
        assert got.dtype == im.dtype and got.shape == want.shape
        assert np.all(got == want), (name, got, want)          # ==: the sign of a zero does not matter


@pytest.mark.parametrize("dtype", DTYPES)
def test_order_statistics_large_bucket_nan_and_argument_errors(dtype):
    from imageanalysis3_amd import _lib as L
    # one bucket holds 491 520 > 2^16 voxels in every pass
    im = np.full((30, 128, 128), 1234, dtype=dtype)
    n = im.size
    with L.DeviceStack.upload(im) as st:
        assert np.all(st.order_stats(_ranks(n)) == 1234)
        assert np.all(st.order_stats(np.arange(16) * (n // 16)) == 1234)     # 16 ranks in one call
        for bad in ([-1], [n], [0] * 17, []):
            with pytest.raises(ValueError):
                st.order_stats(bad)
        for bad in ([-0.5], [100.5], [float("nan")], [50] * 9):
            with pytest.raises(ValueError):
                st.percentiles(bad)
    if dtype == np.float32:   # NaNs of either sign order last, as np.sort puts them
        rng = np.random.RandomState(5)
        im = rng.normal(0., 10., size=(3, 5, 7)).astype(np.float32)
        im.reshape(-1)[[3, 50]] = np.nan
        im.reshape(-1)[77] = -np.nan
        im.reshape(-1)[[4, 60]] = (np.inf, -np.inf)
        ranks = [0, 1, 50, 100, 101, 102, 103, 104]
        with L.DeviceStack.upload(im) as st:
            got = st.order_stats(ranks)
        assert np.array_equal(got, np.sort(im, axis=None)[ranks], equal_nan=True) and np.isnan(got[-3:]).all()
        assert got[-4] == np.inf and got[0] == -np.inf


@pytest.mark.parametrize("dtype", DTYPES)
def test_percentiles_equal_score_at_percentile(dtype):
    from imageanalysis3_amd import _lib as L
    from imageanalysis3_amd.spot_tools.fitting import _score_at_percentile
    for shape, pers in (((3, 5, 7), [2.5, 5, 25, 50, 90, 99.5, 0, 100]),     # 25 and 50 are whole ranks (0.25 * 104 = 26)
                        ((12, 64, 96), [5, 90, 99.9])):
        for name, im in _contents(shape, dtype).items():
            with L.DeviceStack.upload(im) as st:
                got = st.percentiles(pers)
            with np.errstate(invalid="ignore"):   # an infinite order statistic times a zero weight
                want = np.array([_score_at_percentile(im, p) for p in pers], dtype=np.float64)
            assert got.dtype == np.float64 and np.array_equal(got, want, equal_nan=True), (shape, name, got, want)


@pytest.mark.parametrize("name", ["c1_f32", "c1_u16"])
def test_percentile_seeding_of_a_resident_stack_never_downloads(name, monkeypatch):
    """fit_fov_image / _get_seeds_dev with use_percentile on a resident stack reproduce the goldens of
    test_gpu_parity.test_percentile_threshold_and_seed_mask_golden without the host copy."""
    from test_gpu_parity import assert_rows_close, seed_set
    from imageanalysis3_amd import _lib as L
    from imageanalysis3_amd.spot_tools.fitting import fit_fov_image, get_seeds, _get_seeds_dev, _score_at_percentile
    from imageanalysis3_amd.spot_tools.fitting import stack_percentile_threshold
    g = load_golden("seedopts.npz")
    im = build_case(name)

    def no_download(self):
        raise AssertionError("the stack must stay on the device")

    with L.DeviceStack.upload(im) as st:
        monkeypatch.setattr(L.DeviceStack, "download", no_download)
        for per in (95, 99.5, 98):
            want = _score_at_percentile(im, per) - _score_at_percentile(im, (100 - per) / 2)
            th = stack_percentile_threshold(st, per)
            assert isinstance(th, np.float64) and th == want, per
            tag = "%s_per%s" % (name, str(per).replace(".", "p"))
            got = _get_seeds_dev(st, use_percentile=True, th_seed_per=per, return_h=True)
            assert np.array_equal(seed_set(got), seed_set(g[tag])), tag
        got = _get_seeds_dev(st, use_percentile=True, th_seed_per=99.5, return_h=True,
                             sel_center=[s // 2 for s in im.shape], seed_radius=25)
        assert np.array_equal(seed_set(got), seed_set(g[name + "_per_sel"]))
        t = fit_fov_image(st, "647", use_percentile=True, th_seed_per=99.5, max_num_seeds=None, verbose=False)
        assert t.shape == g[name + "_per_table"].shape
        assert_rows_close(t, g[name + "_per_table"])
        # from an ndarray: one upload, the same device entries
        got = get_seeds(im, use_percentile=True, th_seed_per=98, use_dynamic_th=False, return_h=True)
        assert np.array_equal(seed_set(got), seed_set(g["%s_per98_nodyn" % name]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(5, 24, 40), (7, 33, 17)])     # rows of 4-voxel vectors; an odd plane (one by one)
def test_clip_sum_z_equals_the_restatement(shape, dtype):
    from imageanalysis3_amd import _lib as L
    rng = np.random.RandomState(shape[1])
    x = rng.normal(900., 300., size=shape)
    im = np.clip(x, 0, 65535).astype(np.uint16) if dtype == np.uint16 else (x - 800.).astype(np.float32)
    mid = float(np.median(im))
    with L.DeviceStack.upload(im) as st:
        for limits in (None, (mid - 100.7, mid + 250.2000000000007), (mid + 0.5, mid + 0.5), (-1e9, 1e9)):
            with L.clip_sum_z(st, limits) as out:
                got = out.download()
            want = illum_ref.clip_sum_z(im, limits)
            assert got.dtype == np.float64 and np.array_equal(got, want), limits
        with pytest.raises(ValueError):
            L.clip_sum_z(st, (2.0, 1.0))
    assert np.array_equal(illum_ref.clip_sum_z(im, None), im.astype(np.float64).sum(axis=0))


GAUSS_CASES = [((5, 9), 3), ((1, 17), 2.5), ((1, 17), 4), ((17, 1), 2.5), ((17, 1), 4), ((33, 130), 2.5),
               ((64, 96), 60), ((40, 300), 60)]


@pytest.mark.parametrize("shape,sigma", GAUSS_CASES)
def test_gaussian_filter2d_f64_equals_correlate1d(shape, sigma):
    import np_oracle as O
    from imageanalysis3_amd import _lib as L
    rng = np.random.RandomState(int(shape[0] * 1000 + shape[1] + sigma))
    im = rng.normal(20000., 4000., size=shape)
    w, r = L.gaussian_taps(sigma)
    assert r == int(4 * sigma + 0.5)
    want = O.correlate1d(O.correlate1d(im, w, 0), w, 1)
    got = L.gaussian_filter2d_f64(im, sigma)
    assert got.dtype == np.float64 and np.array_equal(got, want)
    with L.DeviceImage64.upload(im) as d_in, L.gaussian_filter2d_f64(d_in, sigma) as d_out:
        assert np.array_equal(d_out.download(), want)
        assert np.array_equal(d_in.download(), im)
    if shape == (33, 130):    # the other border rule and another truncation
        w2, _ = L.gaussian_taps(sigma, 2.0)
        want = O.correlate1d(O.correlate1d(im, w2, 0, "nearest"), w2, 1, "nearest")
        assert np.array_equal(L.gaussian_filter2d_f64(im, sigma, truncate=2.0, mode=L.MODE_NEAREST), want)


def test_gaussian_filter2d_f64_radius_limit():
    from imageanalysis3_amd import _lib as L
    im = np.ones((4, 6))
    assert np.array_equal(L.gaussian_filter2d_f64(im, 256.0), im * L.gaussian_filter2d_f64(im, 256.0)[0, 0])   # radius 1024
    with pytest.raises(NotImplementedError):
        L.gaussian_filter2d_f64(im, 256.25)                                                                    # radius 1025
    with pytest.raises(NotImplementedError):
        L.gaussian_filter2d_f64(im, 1e12)
    with pytest.raises(ValueError):
        L.gaussian_filter2d_f64(im, 0.0)


def test_image_to_profile_equals_the_reference(tmp_path):
    from conftest import write_dax
    from imageanalysis3_amd import _lib as L
    from imageanalysis3_amd.correction_tools import illumination as I
    g = load_golden("illum.npz")
    stacks = illum_ref.prepared_stacks()
    resident = [L.DeviceStack.upload(s) for s in stacks]
    try:
        for key, s, remove_cap, cap, sigma in illum_ref.profile_cases():
            got = I._stack_to_profile(resident[s], remove_cap, cap, sigma)
            assert got.dtype == np.float64 and np.array_equal(got, g[key]), key
        # a float32 stack of the same values gives the same profile; an ndarray is uploaded for the call
        got = I._stack_to_profile(stacks[0].astype(np.float32), True, [0.5, 99.9], 3)
        assert np.array_equal(got, g["prof_s0_sig3_cap2"])
    finally:
        for r in resident:
            r.free()
    # through a .dax file: a two-colour movie whose 647 frames are the prepared stack (no buffer frames; hot pixels and
    # z shift off, so the channel arrives as it is)
    raw = np.full((2 * stacks[1].shape[0],) + stacks[1].shape[1:], 100, np.uint16)
    raw[0::2] = stacks[1]
    path = str(tmp_path / "two_0.dax")
    write_dax(path, raw)
    for key, cap, remove_cap in (("prof_s1_sig3_cap1", [90, 5], True), ("prof_s1_sig60_nocap", [5, 90], False)):
        sigma = 3 if "sig3" in key else 60
        got = I._image_to_profile(path, ['647'], remove_cap, cap, sigma, list(stacks[1].shape), ['647', '488'], 0, 0,
                                  False, 4, False, False)
        assert len(got) == 1 and np.array_equal(got[0], g[key]), key


@pytest.mark.parametrize("zs", [True, False])
def test_generate_illumination_correction_equals_the_reference(zs, tmp_path):
    from imageanalysis3_amd.correction_tools import illumination as I
    from imageanalysis3_amd.io_tools.load import load_correction_profile
    g = load_golden("illum.npz")
    folder = str(tmp_path)
    case = illum_ref.write_movies(folder)
    kw = illum_ref.movie_kwargs(case, zs)
    pfs = I.Generate_illumination_correction(folder, **kw)
    assert len(pfs) == 2
    for ch, pf in zip(illum_ref.MOVIE_CHANNELS, pfs):
        assert pf.dtype == np.float64 and np.array_equal(pf, g["gen_zs%d_%s" % (int(zs), ch)]), ch
    save_folder = os.path.join(folder, "Corrections")
    for ch, pf in zip(illum_ref.MOVIE_CHANNELS, pfs):
        assert np.array_equal(np.load(os.path.join(save_folder, "illumination_correction_%s_64x64.npy" % ch)), pf)
    back = load_correction_profile('illumination', corr_channels=illum_ref.MOVIE_CHANNELS, correction_folder=save_folder,
                                   all_channels=case["chs"], im_size=[case["Z"], case["X"], case["Y"]])
    assert all(np.array_equal(back[ch], pf) for ch, pf in zip(illum_ref.MOVIE_CHANNELS, pfs))
    again = I.Generate_illumination_correction(folder, **dict(kw, overwrite=False))
    assert all(np.array_equal(a, b) for a, b in zip(again, pfs))
    # the other order of channels and a forced recomputation give the same profiles
    swapped = I.Generate_illumination_correction(folder, **dict(kw, sel_channels=['561', '750'], overwrite=True))
    assert np.array_equal(swapped[0], pfs[1]) and np.array_equal(swapped[1], pfs[0])
