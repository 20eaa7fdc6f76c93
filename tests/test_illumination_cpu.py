"""CPU: the NumPy restatement of the illumination-profile generator against the reference's own outputs
(tests/golden/illum.npz), and the host logic of the correction_tools/illumination.py shim."""
import os

import numpy as np
import pytest

from conftest import load_golden
from harness import illum_ref


@pytest.fixture(scope="module")
def golden():
    return load_golden("illum.npz")


def test_restatement_image_profiles_equal_reference(golden):
    stacks = illum_ref.prepared_stacks()
    assert [s.shape for s in stacks] == list(illum_ref.STACK_SHAPES) and all(s.dtype == np.uint16 for s in stacks)
    for key, s, remove_cap, cap, sigma in illum_ref.profile_cases():
        got = illum_ref.image_profile(stacks[s], remove_cap, cap, sigma)
        assert got.dtype == np.float64 and np.array_equal(got, golden[key]), key
    # the cap limits are generally not whole numbers, and either order of the pair gives the same profile
    lims = [v for st in stacks for cap in illum_ref.CAPS for v in illum_ref.cap_limits(st, cap)]
    print("cap limits:", lims)
    assert sum(v != int(v) for v in lims) >= 6
    assert np.array_equal(golden["prof_s1_sig3_cap0"], golden["prof_s1_sig3_cap1"])
    assert not np.array_equal(golden["prof_s1_sig3_cap0"], golden["prof_s1_sig3_nocap"])


@pytest.mark.parametrize("zs", [True, False])
def test_restatement_generated_profiles_equal_reference(golden, zs):
    case, raws = illum_ref.movies_in_order()
    got = illum_ref.generate(raws, case, zs)
    for ch, pf in zip(illum_ref.MOVIE_CHANNELS, got):
        assert np.array_equal(pf, golden["gen_zs%d_%s" % (int(zs), ch)]), ch
        assert pf.max() == 1.0


def test_score_at_percentile_restatement_matches_scipy_and_shim():
    from scipy.stats import scoreatpercentile
    from imageanalysis3_amd.spot_tools.fitting import _score_at_percentile
    rng = np.random.RandomState(2)
    for a in (rng.randint(0, 3000, size=105).astype(np.uint16), rng.normal(0, 50, size=105).astype(np.float32)):
        for per in (0, 2.5, 5, 25, 50, 90, 99.5, 100):
            ref = scoreatpercentile(a, per)
            assert illum_ref.score_at_percentile(a, per) == ref == _score_at_percentile(a, per), per


def test_illumination_correction_arguments():
    from imageanalysis3_amd.correction_tools.illumination import illumination_correction
    rng = np.random.RandomState(0)
    prof = 0.5 + 0.5 * rng.rand(6, 7)
    im3 = rng.randint(0, 65535, size=(3, 6, 7)).astype(np.uint16)
    out = illumination_correction(im3, prof)
    assert out.dtype == np.uint16 and out.shape == im3.shape
    assert np.array_equal(out, np.clip(im3.astype(np.float32) / prof[None], 0, 65535).astype(np.uint16))
    assert out.max() == 65535                                    # clipped to the dtype's range, not wrapped
    out2 = illumination_correction(im3[0], prof)
    assert np.array_equal(out2, out[0])
    with pytest.raises(IndexError):
        illumination_correction(im3, prof[0])
    with pytest.raises(IndexError):
        illumination_correction(im3, prof[None])
    with pytest.raises(IndexError):
        illumination_correction(im3[0, 0], prof)
    with pytest.raises(IndexError):
        illumination_correction(im3[None], prof)


def test_signatures_and_defaults_follow_the_reference():
    import inspect
    from imageanalysis3_amd.correction_tools import illumination as I
    g = inspect.signature(I.Generate_illumination_correction).parameters
    assert list(g) == ["data_folder", "sel_channels", "num_threads", "parallel", "num_images", "single_im_size",
                       "all_channels", "num_buffer_frames", "num_empty_frames", "correction_folder", "hot_pixel_corr",
                       "hot_pixel_th", "z_shift_corr", "remove_cap", "cap_th_per", "gaussian_filter_size", "save",
                       "overwrite", "save_folder", "save_prefix", "make_plot", "verbose"]
    assert (g["num_threads"].default, g["parallel"].default, g["num_images"].default) == (12, True, 48)
    assert (g["gaussian_filter_size"].default, g["z_shift_corr"].default, g["make_plot"].default) == (60, True, True)
    assert g["cap_th_per"].default == [5, 90] and g["save_prefix"].default == 'illumination_correction_'
    p = inspect.signature(I._image_to_profile).parameters
    assert list(p) == ["filename", "sel_channels", "remove_cap", "cap_th_per", "gaussian_filter_size", "single_im_size",
                       "all_channels", "num_buffer_frames", "num_empty_frames", "hot_pixel_corr", "hot_pixel_th",
                       "z_shift_corr", "verbose"]
    assert (p["gaussian_filter_size"].default, p["z_shift_corr"].default, p["num_buffer_frames"].default) == (40, False, 10)
    assert list(inspect.signature(I.illumination_correction).parameters) == ["im", "corr_profile"]


def _driver(monkeypatch, tmp_path, names, **kw):
    """Generate_illumination_correction with the device work replaced: per image a profile that encodes the file."""
    from imageanalysis3_amd.correction_tools import illumination as I
    seen = []

    def fake_profile(filename, sel_channels, *a, **k):
        seen.append((os.path.basename(filename), list(sel_channels)))
        v = int(os.path.basename(filename).split('.dax')[0].split('_')[-1])
        return [np.full((4, 6), float(v * 10 + int(ch)), dtype=np.float64) for ch in sel_channels]

    monkeypatch.setattr(I, "_image_to_profile", fake_profile)
    monkeypatch.setattr(I, "_gaussian_filter_f64", lambda im, sigma: np.asarray(im, dtype=np.float64) + 1.0)
    for n in names:
        (tmp_path / n).write_bytes(b"")
    out = I.Generate_illumination_correction(str(tmp_path), single_im_size=[3, 4, 6],
                                             all_channels=['750', '647', '561'], verbose=False, **kw)
    return out, seen


def test_driver_file_order_names_and_limits(monkeypatch, tmp_path):
    names = ["Conv_zscan_10.dax", "Conv_zscan_2.dax", "Conv_zscan_1.dax", "Conv_zscan_3.inf", "notes_7.txt"]
    out, seen = _driver(monkeypatch, tmp_path, names, sel_channels=['561', '750'], num_images=2, make_plot=False)
    assert seen == [("Conv_zscan_1.dax", ['561', '750']), ("Conv_zscan_2.dax", ['561', '750'])]   # integer order, 2 of 3
    folder = tmp_path / "Corrections"                                     # the default save folder is created
    assert sorted(os.listdir(folder)) == ["illumination_correction_561_4x6.npy", "illumination_correction_750_4x6.npy"]
    # mean over the images, "filter" (+1), divided by the maximum: constant images give all ones
    assert len(out) == 2 and all(o.shape == (4, 6) and np.array_equal(o, np.ones((4, 6))) for o in out)
    assert np.array_equal(np.load(folder / "illumination_correction_561_4x6.npy"), out[0])


def test_driver_loads_existing_files_without_the_library(monkeypatch, tmp_path):
    from imageanalysis3_amd import _lib
    from imageanalysis3_amd.correction_tools import illumination as I
    folder = tmp_path / "saved"
    folder.mkdir()
    a, b = np.arange(24.).reshape(4, 6), np.arange(24.).reshape(4, 6)[::-1].copy()
    np.save(folder / "pf_750_4x6.npy", a)
    np.save(folder / "pf_561_4x6.npy", b)

    def no_library(*args, **kw):
        raise AssertionError("the library must not be loaded")

    monkeypatch.setattr(_lib, "lib", no_library)
    monkeypatch.setattr(I, "_image_to_profile", no_library)
    out = I.Generate_illumination_correction(str(tmp_path), sel_channels=['561', '750'], single_im_size=[3, 4, 6],
                                             save_folder=str(folder), save_prefix="pf_", make_plot=False, verbose=False)
    assert np.array_equal(out[0], b) and np.array_equal(out[1], a)       # the order of sel_channels
    # one channel on file, one computed: the returned list still follows sel_channels; overwrite recomputes both
    monkeypatch.undo()
    os.remove(folder / "pf_561_4x6.npy")
    out, seen = _driver(monkeypatch, tmp_path, ["m_4.dax"], sel_channels=['561', '750'], save_folder=str(folder),
                        save_prefix="pf_", make_plot=False)
    assert seen == [("m_4.dax", ['561'])] and np.array_equal(out[1], a) and np.array_equal(out[0], np.ones((4, 6)))
    monkeypatch.undo()
    out, seen = _driver(monkeypatch, tmp_path, [], sel_channels=['561', '750'], save_folder=str(folder),
                        save_prefix="pf_", make_plot=False, overwrite=True)
    assert seen == [("m_4.dax", ['561', '750'])] and np.array_equal(np.load(folder / "pf_750_4x6.npy"), out[1])


def test_driver_plots_without_showing(monkeypatch, tmp_path, capsys):
    try:
        import matplotlib  # noqa: F401
        have_mpl = True
    except ImportError:
        have_mpl = False
    out, _ = _driver(monkeypatch, tmp_path, ["m_1.dax"], sel_channels=['647'], make_plot=True)
    assert os.path.isfile(tmp_path / "Corrections" / "illumination_correction_647_4x6.png") == have_mpl
    monkeypatch.undo()
    # nothing saved: no figure, no error (make_plot=True is the reference's default)
    out, _ = _driver(monkeypatch, tmp_path, [], sel_channels=['647'], make_plot=True, save=False, overwrite=True,
                     save_folder=str(tmp_path / "none"))
    assert not [f for f in os.listdir(tmp_path / "none") if f.endswith(".png")]
