"""CPU: the NumPy restatement of the chromatic-profile generator against the reference's own outputs
(tests/golden/chromatic*.npz), and the host logic of io_tools/crop.py and correction_tools/chromatic.py with the device
calls replaced by that restatement."""
import json
import os
import pickle
import re

import numpy as np
import pytest

from conftest import load_golden
from harness import chrom_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return load_golden("chromatic.npz")


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(ROOT, "tests", "golden", "chromatic.json")) as f:
        return json.load(f)


def test_restatement_crops_equal_reference(golden):
    stacks, f32 = R.crop_stacks()
    assert [a.shape for a, _ in stacks] == list(R.CROP_STACK_SHAPES)
    n = 0
    for k, (a, b) in enumerate(stacks):
        for name, ca, cb in R.crop_centres(k):
            for s, size in enumerate(R.CROP_SIZES):
                key = "crop_s%d_%s_c%d" % (k, name, s)
                for im, c, tag in ((a, ca, "_a"), (b, cb, "_b")) + (((f32, ca, "_f32"),) if k == 0 else ()):
                    got = R.crop_neighboring_area(im, c, size)
                    assert got.dtype == golden[key + tag].dtype and np.array_equal(got, golden[key + tag]), key + tag
                    n += 1
    assert n == (14 * 3 + 4 * 2) * 4


def test_fixture_covers_every_rough_crop_case():
    """Clipped at each face, on both sides in z, whole and half-integer centres (floor and ceil coincide)."""
    seen = set()
    for k, shape in enumerate(R.CROP_STACK_SHAPES):
        for name, ca, cb in R.crop_centres(k):
            for size in R.CROP_SIZES:
                left, right, t = R.rough_crop(shape, ca, size)
                full = R.box_sizes(size)
                for a in range(3):
                    lo_clip, hi_clip = ca[a] - full[a] / 2 < 0, ca[a] + full[a] / 2 > shape[a]
                    seen.add((a, bool(lo_clip), bool(hi_clip)))
                    if (ca[a] - full[a] / 2) == np.floor(ca[a] - full[a] / 2) and not lo_clip and not hi_clip:
                        seen.add("exact")
                        assert right[a] - left[a] == full[a]
    for a in range(3):
        assert (a, True, False) in seen and (a, False, True) in seen and (a, False, False) in seen
    assert (0, True, True) in seen and "exact" in seen


def test_movie_fixtures_have_distinct_seed_heights(recorded):
    """Seed heights are whole numbers on uint16 images; two equal ones would leave the order of the fitted spots, and
    so of the pairs, to the sort (the reference's is not stable).  The movies are chosen to have none."""
    import np_oracle as O
    gaps = []
    for k in range(len(R.MOVIE_NAMES)):
        ref, _, ca, _, _ = R.movie_pair(k)
        for im in (ref, ca):
            h = O.get_seeds(im, th_seed=R.FITTING_ARGS['th_seed'], return_h=True)[:, 3]
            gaps.append(float(np.diff(np.sort(h)).min()))
    assert min(gaps) > 0 and min(gaps) == recorded["conditions"]["seed_height_min_gap"]


def test_restatement_equals_scipy_far_outside():
    """Positions more than 12 samples outside the rough crop are clamped to the padded array (a box of 15 at a face)."""
    a = R.crop_stacks()[0][0][0]
    for c in ((-6.9, 20.2, 40.1), (5.0, 46.4, -7.2)):
        assert np.array_equal(R.crop_neighboring_area(a, c, 15), R.crop_by_scipy(a, c, 15)), c


def test_regression_restatement_within_recorded_tolerance(golden, recorded):
    """The float64 formulas on exact sums (what the kernel evaluates) against exact rational arithmetic."""
    tol = recorded["tolerances"]["regression_rel"]
    for key in golden:
        if key.endswith("_reg"):
            xa, xb = golden[key[:-4] + "_a"], golden[key[:-4] + "_b"]
            exact = R.regression_exact(xa, xb)
            for q, v, e in zip(("slope", "intercept", "rsq"), R.regression_f64(xa, xb), exact):
                assert R.rel_distance(v, e) <= 16 * tol[q], (key, q)
            for q, v, e in zip(("slope", "intercept", "rsq"), golden[key], exact):   # the fixture's own distance
                assert R.rel_distance(v, e) <= tol[q], (key, q)
    const, ramp = np.full((4, 4, 4), 7, np.uint16), np.arange(64, dtype=np.uint16).reshape(4, 4, 4)
    assert R.regression_f64(const, ramp) == (0.0, 31.5, 0.0)
    assert R.regression_f64(ramp, const) == (0.0, 7.0, 1.0)
    assert R.regression_f64(const, const) == (0.0, 7.0, 1.0)


def _field_golden(golden, s, order):
    if s == 1 and order > 0:
        return load_golden("chromatic_field_o%d.npz" % order)["poly_s1_o%d" % order]
    return golden["poly_s%d_o%d" % (s, order)]


def test_restatement_fields_within_bound_of_reference(golden):
    from imageanalysis3_amd.correction_tools.chromatic import generate_polynomial_data
    for s, (shape, center) in enumerate(zip(R.POLY_SHAPES, R.POLY_CENTERS)):
        for order in range(4):
            c = R.poly_constants(s, order)
            assert len(c) == R.poly_columns(order)
            got = R.poly_field(shape, center, order, c)
            want = _field_golden(golden, s, order)
            assert got.shape == want.shape and np.all(np.abs(got - want) <= R.poly_bound(shape, center, order, c)), (s, order)
            if s == 0:   # the columns are generate_polynomial_data's, bit for bit
                grid = np.indices(shape).reshape(3, -1) - np.array(center)[:, None]
                cols = generate_polynomial_data(grid.T, order)
                assert np.array_equal(cols, np.array([m.ravel() for m in R.poly_monomials(shape, center, order)]).T)


def test_exports_agree_with_header():
    from imageanalysis3_amd import _lib
    src = open(os.path.join(ROOT, "include", "ia3.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(ia3_[a-z0-9_]+)\s*\(", src))
    new = {"ia3_crop_pairs_dev", "ia3_poly_field_dev", "ia3_buffer_alloc", "ia3_buffer_download"}
    assert new <= declared and new <= set(_lib.EXPORTS)
    lib = _lib.lib()
    assert all(hasattr(lib, n) for n in new)


def test_argument_errors_before_device():
    from imageanalysis3_amd import _lib as L
    from imageanalysis3_amd.io_tools.crop import crop_neighboring_area, crop_neighboring_areas
    from imageanalysis3_amd.correction_tools import chromatic as ch
    im = np.zeros((6, 8, 8), dtype=np.uint16)
    with pytest.raises(TypeError):
        crop_neighboring_area([[1, 2], [3, 4]], [1, 1, 1], 3)
    with pytest.raises(NotImplementedError):
        crop_neighboring_area(im, [1, 1, 1], 3, extrapolate_mode='reflect')
    for bad in (0, 16, [3, 0, 3], [3, 3, 16]):
        with pytest.raises(ValueError):
            crop_neighboring_area(im, [1, 1, 1], bad)
    with pytest.raises(TypeError):
        crop_neighboring_area(im, [1, 1, 1], 3.5)
    with pytest.raises(ValueError):
        crop_neighboring_areas(im, [1, 1, 1], 3)

    class Fake(object):
        def __init__(self, shape, dtype):
            self.shape, self.dtype, self._h = shape, np.dtype(dtype), None
    for other in (Fake((6, 8, 9), np.uint16), Fake((6, 8, 8), np.float32)):
        with pytest.raises(ValueError):
            L.crop_pairs(Fake((6, 8, 8), np.uint16), np.ones((2, 3)), [3, 3, 3], other, np.ones((2, 3)))
    with pytest.raises(ValueError):
        L.crop_pairs(Fake((6, 8, 8), np.uint16), np.ones((2, 3)), [3, 3, 3], Fake((6, 8, 8), np.uint16), np.ones((3, 3)))
    info = {'constants': [np.zeros(4), np.zeros(4), np.zeros(1)], 'fitting_orders': [1, 1, 0], 'ref_center': np.zeros(3)}
    with pytest.raises(NotImplementedError):
        ch.chromatic_profile_from_constants(dict(info, constants=[np.zeros(35)] + info['constants'][1:], fitting_orders=[4, 1, 0]), (4, 4, 4))
    with pytest.raises(ValueError):
        ch.chromatic_profile_from_constants(dict(info, constants=[np.zeros(3)] + info['constants'][1:]), (4, 4, 4))
    with pytest.raises(ValueError):
        ch.chromatic_profile_from_constants(info, (4, 4))
    with pytest.raises(TypeError):
        ch.chromatic_profile_from_constants(3.0, (4, 4, 4))
    with pytest.raises(TypeError):
        L.poly_field(info['constants'], [1, 1, 0], np.zeros(3), (4, 4, 4), np.float16)


class _HostStack(object):
    """What the stubbed device calls pass around instead of a resident stack."""
    def __init__(self, im):
        self.im, self.shape, self.dtype = im, im.shape, im.dtype

    def free(self):
        pass


@pytest.fixture()
def stubbed(monkeypatch):
    """correction_tools/chromatic.py with every device call replaced: prepared stacks, fits of the golden centres'
    kind (the true spot positions), boxes and regressions from chrom_ref, the field from chrom_ref."""
    from imageanalysis3_amd import _lib as L
    from imageanalysis3_amd.correction_tools import chromatic as ch
    from imageanalysis3_amd.io_tools.load import DeviceBuffer
    calls = {"crop_pairs": 0, "poly_field": 0, "correct": 0}
    prepared = R.prepared_correct_fov_image(upload=_HostStack)

    def correct(filename, sel_channels, **kw):
        calls["correct"] += 1
        assert kw.get("return_device") is True and kw.get("warp_image") is False
        out = prepared(filename, sel_channels, **kw)
        out[0][0].spots = (R.MOVIE_NAMES.index(os.path.basename(filename)), str(sel_channels[0]) == R.REF_CHANNEL)
        return out

    def fit(im, channel, **kw):   # rows of the true centres: [h, z, x, y, ...]
        k, is_ref = im.spots
        centers, moved, heights = R.movie_spots(k)
        rows = np.zeros((len(centers), 11), dtype=np.float32)
        rows[:, 0], rows[:, 1:4] = heights, centers if is_ref else moved
        return rows

    def crop_pairs(a, ca, crop, b=None, cb=None, regress=False):
        calls["crop_pairs"] += 1
        xa = np.array([R.crop_neighboring_area(a.im, c, list(crop)) for c in ca])
        xb = np.array([R.crop_neighboring_area(b.im, c, list(crop)) for c in cb])
        reg = np.array([R.regression_f64(p, q) for p, q in zip(xa, xb)])
        return xa, xb, (reg[:, 0].copy(), reg[:, 1].copy(), reg[:, 2].copy())

    class FakeBuffer(object):
        def __init__(self, arr):
            self.arr, self.shape, self.dtype = arr, arr.shape, arr.dtype

        def download(self):
            return self.arr.copy()

        def free(self):
            pass

    def poly_field(consts, orders, center, shape, dtype=np.float64):
        calls["poly_field"] += 1
        return np.array([R.poly_field(shape, center, o, c) for c, o in zip(consts, orders)]).astype(dtype)

    monkeypatch.setattr(ch, "correct_fov_image", correct)
    monkeypatch.setattr(ch, "fit_fov_image", fit)
    monkeypatch.setattr(L, "crop_pairs", crop_pairs)
    monkeypatch.setattr(L, "poly_field", poly_field)
    monkeypatch.setattr(DeviceBuffer, "adopt", classmethod(lambda cls, p, shape, dtype: FakeBuffer(p)))
    return ch, calls


def test_spot_pairs_schema_and_temp_file(stubbed, tmp_path, recorded):
    ch, calls = stubbed
    ca, ref = R.make_folders(str(tmp_path))
    args = (os.path.join(ca, R.MOVIE_NAMES[0]), os.path.join(ref, R.MOVIE_NAMES[0]), R.CA_CHANNEL, R.REF_CHANNEL, R.BEAD_CHANNEL)
    kw = dict(correction_args=R.correction_args(), fitting_args=dict(R.FITTING_ARGS), rsq_th=R.RSQ_TH, verbose=False)
    infos = ch.find_chromatic_spot_pairs(*args, **kw)
    assert calls["crop_pairs"] == 1 and calls["correct"] == 2          # one device call for all pairs
    assert 30 <= len(infos) <= 50 - R.N_POOR
    for i in infos:
        assert {k: type(v).__name__ for k, v in i.items()} == recorded["types"]
        assert i["ref_im"].dtype == np.uint16 and i["ref_im"].shape == (9, 9, 9) and i["ca_im"].shape == (9, 9, 9)
        assert i["slope"].shape == (1,) and i["slope"].dtype == np.float64 and i["rsquare"] >= R.RSQ_TH
        assert i["ref_coord"].dtype == np.float32 and i["ca_coord"].shape == (3,)
        assert np.array_equal(i["drift"], R.movie_drift(0))
        assert i["ca_file"] == args[0] and i["ref_file"] == args[1]
    temp = os.path.join(ca, "chromatic_Conv_zscan_2_channel_750_ref_647.pkl")
    assert os.path.isfile(temp)
    with open(temp, "rb") as f:
        assert len(pickle.load(f)) == len(infos)
    # the temp file is read back instead of computed; overwrite computes again; save_temp=False writes nothing
    again = ch.find_chromatic_spot_pairs(*args, **kw)
    assert calls["crop_pairs"] == 1 and len(again) == len(infos)
    ch.find_chromatic_spot_pairs(*args, overwrite=True, **kw)
    assert calls["crop_pairs"] == 2
    os.remove(temp)
    ch.find_chromatic_spot_pairs(*args, save_temp=False, **kw)
    assert calls["crop_pairs"] == 3 and not os.path.isfile(temp)


@pytest.mark.parametrize("verbose", [True, False])
def test_generate_selects_files_and_saves_only_when_verbose(stubbed, tmp_path, verbose, capsys):
    ch, calls = stubbed
    ca, ref = R.make_folders(str(tmp_path))
    kw = dict(parallel=True, num_threads=3, correction_args=R.correction_args(), fitting_args=dict(R.FITTING_ARGS),
              rsq_th=R.RSQ_TH, make_plots=False, verbose=verbose)
    pfs, consts = ch.Generate_chromatic_abbrevation(ca, ref, R.CA_CHANNEL, R.REF_CHANNEL, R.BEAD_CHANNEL,
                                                    fitting_orders=[1, 2, 0], **kw)
    capsys.readouterr()
    assert calls["crop_pairs"] == 3 and calls["poly_field"] == 1       # the movie only one folder holds is left out
    temps = sorted(f for f in os.listdir(ca) if f.startswith("chromatic_Conv"))
    assert temps == sorted("chromatic_Conv_zscan_%d_channel_750_ref_647.pkl" % k for k in (1, 2, 10))
    assert len(pfs) == 3 and all(p.shape == R.MOVIE_SHAPE and p.dtype == np.float64 for p in pfs)
    assert [len(c) for c in consts] == [4, 10, 1]
    # a first-order field was put in: its slopes come back (shift = ca + drift - ref = chromatic_shift)
    assert abs(consts[0][2] - 0.004) < 2e-4 and abs(consts[1][2] - 0.012) < 5e-4 and abs(consts[1][3] + 0.003) < 5e-4
    base = os.path.join(ca, "chromatic_correction_750_647_20_96_96")
    made = sorted(f for f in os.listdir(ca) if f.startswith("chromatic_correction"))
    if not verbose:
        assert made == []                                               # the reference saves under `if verbose:`
        return
    assert made == [os.path.basename(base) + ".npy", os.path.basename(base) + "_const.pkl"]
    assert np.array_equal(np.load(base + ".npy"), np.array(pfs))
    with open(base + "_const.pkl", "rb") as f:
        cd = pickle.load(f)
    assert sorted(cd) == ["constants", "fitting_orders", "ref_center", "rsquares"]
    assert np.array_equal(cd["ref_center"], np.array(R.MOVIE_SHAPE) / 2) and list(cd["fitting_orders"]) == [1, 2, 0]
    # load-if-exists: nothing is computed, the saved arrays come back
    pfs2, consts2 = ch.Generate_chromatic_abbrevation(ca, ref, R.CA_CHANNEL, R.REF_CHANNEL, R.BEAD_CHANNEL,
                                                      fitting_orders=3, **kw)
    capsys.readouterr()
    assert calls["poly_field"] == 1 and np.array_equal(np.array(pfs2), np.array(pfs))
    assert all(np.array_equal(a, b) for a, b in zip(consts2, consts))


def test_generate_start_fov_num_images_orders_and_plots(stubbed, tmp_path):
    ch, calls = stubbed
    ca, ref = R.make_folders(str(tmp_path))
    kw = dict(correction_args=R.correction_args(), fitting_args=dict(R.FITTING_ARGS), rsq_th=R.RSQ_TH, verbose=False)
    with pytest.raises(TypeError):
        ch.Generate_chromatic_abbrevation(ca, ref, R.CA_CHANNEL, R.REF_CHANNEL, R.BEAD_CHANNEL, fitting_orders=1.0,
                                          make_plots=False, **kw)
    n0 = calls["crop_pairs"]
    for f in os.listdir(ca):
        if f.endswith(".pkl"):
            os.remove(os.path.join(ca, f))
    out = str(tmp_path / "out")
    os.makedirs(out)
    pfs, consts = ch.Generate_chromatic_abbrevation(ca, ref, R.CA_CHANNEL, R.REF_CHANNEL, R.BEAD_CHANNEL, start_fov=1,
                                                    num_images=1, fitting_orders=np.int32(1), ref_center=[9.5, 40.0, 50.0],
                                                    save_folder=out, save_name="ca", make_plots=True, save_plots=True, **kw)
    assert calls["crop_pairs"] == n0 + 1                                # names sorted by number: 1, [2], 10
    assert sorted(f for f in os.listdir(ca) if f.endswith(".pkl")) == ["chromatic_Conv_zscan_2_channel_750_ref_647.pkl"]
    assert [len(c) for c in consts] == [4, 4, 4]
    import importlib.util
    if importlib.util.find_spec("matplotlib") is not None:
        assert sorted(os.listdir(out)) == ["ca_750_647_20_96_96_%d.png" % i for i in range(3)]


def test_device_buffer_shape_checks_use_shape():
    """The four shape checks of io_tools/load.py read DeviceBuffer.shape: a buffer made on the device has no host array."""
    src = open(os.path.join(ROOT, "imageanalysis3_amd", "io_tools", "load.py")).read()
    assert ".arr.shape" not in src.split("def _as_buffer")[1]
    from imageanalysis3_amd.io_tools.load import DeviceBuffer
    b = DeviceBuffer.adopt(None, (3, 4, 5, 6), np.float32)
    assert b.shape == (3, 4, 5, 6) and b.dtype == np.float32 and b.dtype_code == 1 and b.arr is None
    assert DeviceBuffer.adopt(None, (2, 2), np.float64).dtype_code == 2
    with pytest.raises(TypeError):
        DeviceBuffer.adopt(None, (2, 2), np.uint16)
