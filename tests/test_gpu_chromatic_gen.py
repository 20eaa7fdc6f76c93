"""GPU: the sub-pixel boxes and regressions of ia3_crop_pairs_dev, the dense polynomial field of ia3_poly_field_dev
(csrc/calib.hip) and the chromatic-profile generator built on them (correction_tools/chromatic.py, io_tools/crop.py).

Boxes are compared bit for bit with the reference's own (tests/golden/chromatic.npz); regressions with exact rational
arithmetic on the golden boxes, within 16 times the reference's own recorded distance from it; fields bit for bit with
the sequential statement of tests/harness/chrom_ref.py and, within n_cols * 2^-52 * sum |C_k m_k| (which bounds the
difference between any two summation orders), with the reference's np.dot; the two generator functions with the
reference's outputs within twice the change the reference itself shows when the paired centres move by 1e-4 relative
(tests/golden/chromatic.json)."""
import json
import os
import pickle

import numpy as np
import pytest

from conftest import load_golden, build_chain_case, chain_kwargs
from harness import chrom_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QS = ("slope", "intercept", "rsq")


@pytest.fixture(scope="module")
def golden():
    return load_golden("chromatic.npz")


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(ROOT, "tests", "golden", "chromatic.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def stacks():
    return R.crop_stacks()


@pytest.mark.parametrize("k", [0, 1])
def test_crops_and_regressions_match_reference(golden, recorded, stacks, k):
    from imageanalysis3_amd import _lib as L
    tol = recorded["tolerances"]["regression_rel"]
    a, b = stacks[0][k]
    cases = R.crop_centres(k)
    ca, cb = np.array([c[1] for c in cases]), np.array([c[2] for c in cases])
    worst = dict.fromkeys(QS, 0.0)
    with L.DeviceStack.upload(a) as sa, L.DeviceStack.upload(b) as sb:
        for s, size in enumerate(R.CROP_SIZES):
            xa, xb, reg = L.crop_pairs(sa, ca, R.box_sizes(size), sb, cb, regress=True)
            assert xa.dtype == np.uint16 and xa.shape == (len(cases),) + tuple(R.box_sizes(size))
            for i, (name, _, _) in enumerate(cases):
                key = "crop_s%d_%s_c%d" % (k, name, s)
                assert np.array_equal(xa[i], golden[key + "_a"]), key
                assert np.array_equal(xb[i], golden[key + "_b"]), key
                exact = R.regression_exact(golden[key + "_a"], golden[key + "_b"])
                for q, v, e in zip(QS, (reg[0][i], reg[1][i], reg[2][i]), exact):
                    dist = R.rel_distance(v, e)
                    worst[q] = max(worst[q], dist)
                    assert dist <= 16 * tol[q], (key, q, dist, tol[q])
    print("largest relative distance from the exact regression:", worst, "allowed:", {q: 16 * tol[q] for q in QS})


def test_float32_crops_and_the_single_box_interface(golden, stacks):
    from imageanalysis3_amd import _lib as L
    from imageanalysis3_amd.io_tools.crop import crop_neighboring_area, crop_neighboring_areas
    f32 = stacks[1]
    cases = R.crop_centres(0)
    ca = np.array([c[1] for c in cases])
    with L.DeviceStack.upload(f32) as st:
        for s, size in enumerate(R.CROP_SIZES):
            got = crop_neighboring_areas(st, ca, size)
            assert got.dtype == np.float32
            for i, (name, _, _) in enumerate(cases):
                assert np.array_equal(got[i], golden["crop_s0_%s_c%d_f32" % (name, s)]), (name, s)
        one = crop_neighboring_area(st, ca[3], np.array([5, 9, 9]))
        assert np.array_equal(one, golden["crop_s0_%s_c3_f32" % cases[3][0]])
        with pytest.raises(NotImplementedError):    # a regression of float32 boxes is not built
            L.crop_pairs(st, ca, [9, 9, 9], st, ca, regress=True)
        with pytest.raises(ValueError):             # the rough crop does not meet the image
            crop_neighboring_area(st, [5.0, 20.0, 60.0], 9)
    a = stacks[0][0][0]
    assert np.array_equal(crop_neighboring_area(a, list(ca[0]), 9), golden["crop_s0_interior_c0_a"])     # ndarray, np.int
    assert np.array_equal(crop_neighboring_area(a, ca[0], np.int32(4)), golden["crop_s0_interior_c2_a"])
    far = (-6.9, 20.2, 40.1)                        # positions clamped to the padded array: a box of 15 at a face
    assert np.array_equal(crop_neighboring_area(a, far, 15), R.crop_by_scipy(a, far, 15))


def test_batches_equal_single_calls(stacks):
    """1, 63, 65 and 300 pairs in one call give the boxes and regressions of 300 calls of one pair."""
    from imageanalysis3_amd import _lib as L
    a, b = stacks[0][0]
    u = np.random.RandomState(5).rand(300, 3)
    ca = u * (np.array(a.shape) - 1.0)
    ca[::7] = np.round(ca[::7])                     # whole and half-integer centres among them
    ca[3::11] = np.floor(ca[3::11]) + 0.5
    cb = np.clip(ca + 0.4 * (np.random.RandomState(6).rand(300, 3) - 0.5), 0, np.array(a.shape) - 1.0)
    size = [5, 9, 9]
    with L.DeviceStack.upload(a) as sa, L.DeviceStack.upload(b) as sb:
        singles = [L.crop_pairs(sa, ca[i:i + 1], size, sb, cb[i:i + 1], regress=True) for i in range(300)]
        xa = np.concatenate([s[0] for s in singles])
        xb = np.concatenate([s[1] for s in singles])
        reg = [np.concatenate([s[2][q] for s in singles]) for q in range(3)]
        for n in (1, 63, 65, 300):
            ga, gb, greg = L.crop_pairs(sa, ca[:n], size, sb, cb[:n], regress=True)
            assert np.array_equal(ga, xa[:n]) and np.array_equal(gb, xb[:n]), n
            assert all(np.array_equal(greg[q], reg[q][:n]) for q in range(3)), n
        only_a = L.crop_pairs(sa, ca, size)
        assert np.array_equal(only_a[0], xa) and only_a[1] is None and only_a[2] is None
    for i in (0, 7, 14, 299):                        # and they are the restatement's boxes
        assert np.array_equal(xa[i], R.crop_neighboring_area(a, ca[i], size)), i
        assert (reg[0][i], reg[1][i], reg[2][i]) == R.regression_f64(xa[i], xb[i])


def test_degenerate_regressions():
    from imageanalysis3_amd import _lib as L
    shape = (8, 16, 16)
    const = np.full(shape, 700, np.uint16)
    noise = np.random.RandomState(2).randint(300, 900, size=shape).astype(np.uint16)
    c = np.array([[3.3, 7.6, 8.1]])
    with L.DeviceStack.upload(const) as sc, L.DeviceStack.upload(noise) as sn:
        xa, xb, (sl, ic, rs) = L.crop_pairs(sc, c, [5, 5, 5], sn, c, regress=True)     # constant x
        assert np.all(xa == 700) and (sl[0], ic[0], rs[0]) == (0.0, float(xb.astype(np.int64).sum()) / 125, 0.0)
        xa, xb, (sl, ic, rs) = L.crop_pairs(sn, c, [5, 5, 5], sc, c, regress=True)     # constant y
        assert (sl[0], ic[0], rs[0]) == (0.0, 700.0, 1.0)
        xa, xb, (sl, ic, rs) = L.crop_pairs(sc, c, [5, 5, 5], sc, c + 0.2, regress=True)   # both constant
        assert (sl[0], ic[0], rs[0]) == (0.0, 700.0, 1.0)


def _field_golden(golden, s, order):
    if s == 1 and order > 0:
        return load_golden("chromatic_field_o%d.npz" % order)["poly_s1_o%d" % order]
    return golden["poly_s%d_o%d" % (s, order)]


def _device_field(consts, orders, center, shape, dtype):
    from imageanalysis3_amd import _lib as L
    from imageanalysis3_amd.io_tools.load import DeviceBuffer
    buf = DeviceBuffer.adopt(L.poly_field(consts, orders, center, shape, dtype), (3,) + tuple(shape), dtype)
    try:
        return buf.download()
    finally:
        buf.free()


@pytest.mark.parametrize("s", [0, 1])
def test_poly_field_matches_statement_and_reference(golden, s):
    shape, center = R.POLY_SHAPES[s], R.POLY_CENTERS[s]
    for o in range(4):
        orders = [o, (o + 1) % 4, (o + 3) % 4]       # every axis meets every order
        consts = [R.poly_constants(s, k) for k in orders]
        f64 = _device_field(consts, orders, center, shape, np.float64)
        f32 = _device_field(consts, orders, center, shape, np.float32)
        assert f64.dtype == np.float64 and f32.dtype == np.float32 and f64.shape == (3,) + shape
        assert np.array_equal(f32, f64.astype(np.float32))                  # the float64 value rounded once
        for a, k in enumerate(orders):
            assert np.array_equal(f64[a], R.poly_field(shape, center, k, consts[a])), (o, a)
            bound = R.poly_bound(shape, center, k, consts[a])
            assert np.all(np.abs(f64[a] - _field_golden(golden, s, k)) <= bound), (o, a)


@pytest.mark.parametrize("shape", [(2, 3, 6), (1, 2, 1100), (2, 3, 1027)])
def test_poly_field_store_paths(shape):
    """Rows that keep 16-byte alignment for float64 only, for both dtypes over several blocks, and for neither."""
    center = (0.4, 1.3, shape[2] / 3.0)
    orders = [3, 2, 1]
    consts = [R.poly_constants(0, k) for k in orders]
    f64 = _device_field(consts, orders, center, shape, np.float64)
    assert all(np.array_equal(f64[a], R.poly_field(shape, center, k, consts[a])) for a, k in enumerate(orders))
    assert np.array_equal(_device_field(consts, orders, center, shape, np.float32), f64.astype(np.float32))


def test_field_arguments():
    from imageanalysis3_amd import _lib as L
    c1 = [np.zeros(4)] * 3
    with pytest.raises(NotImplementedError):
        L.poly_field([np.zeros(35), np.zeros(4), np.zeros(4)], [4, 1, 1], np.zeros(3), (2, 2, 2))
    with pytest.raises(ValueError):
        L.poly_field([np.zeros(5), np.zeros(4), np.zeros(4)], [1, 1, 1], np.zeros(3), (2, 2, 2))
    with pytest.raises(ValueError):
        L.poly_field(c1, [1, 1, 1], np.zeros(3), (2, 0, 2))


def test_profile_from_constants_feeds_the_warps():
    from imageanalysis3_amd.correction_tools.chromatic import chromatic_profile_from_constants
    from imageanalysis3_amd.correction_tools.translate import warp_3d_image
    from imageanalysis3_amd.io_tools.load import correct_fov_image
    case = build_chain_case()
    shape = (case["Z"], case["X"], case["Y"])
    info = {'constants': [R.poly_constants(1, 1), R.poly_constants(1, 2), R.poly_constants(1, 0)],
            'fitting_orders': np.array([1, 2, 0]), 'ref_center': np.array(shape) / 2}
    sel, kw = chain_kwargs(case, "full")
    for dtype in (np.float64, np.float32):
        buf = chromatic_profile_from_constants(info, shape, dtype)
        wrong = chromatic_profile_from_constants(info, (shape[0], shape[1], shape[2] + 2), dtype)
        try:
            assert buf.shape == (3,) + shape and buf.dtype == dtype and buf.arr is None
            host = buf.download()
            assert host.dtype == dtype and np.abs(host).max() > 0.05
            im = case["raw"][2:2 + 4 * shape[0]:4].copy()
            want = warp_3d_image(im, case["drift"], host, warp_order=3, border_mode='nearest')
            assert np.array_equal(warp_3d_image(im, case["drift"], buf, warp_order=3, border_mode='nearest'), want)
            with pytest.raises(IndexError):
                warp_3d_image(im, case["drift"], wrong, warp_order=3, border_mode='nearest')
            ims_h = correct_fov_image(case["raw"], sel, **dict(kw, chromatic_profile={'750': host, '647': None, '561': host}))[0]
            ims_d = correct_fov_image(case["raw"], sel, **dict(kw, chromatic_profile={'750': buf, '647': None, '561': buf}))[0]
            assert all(np.array_equal(x, y) for x, y in zip(ims_h, ims_d))
            with pytest.raises(IndexError):
                correct_fov_image(case["raw"], sel, **dict(kw, chromatic_profile={'750': wrong, '647': None, '561': wrong}))
        finally:
            buf.free()
            wrong.free()


@pytest.fixture()
def prepared(monkeypatch):
    """correction_tools/chromatic.py with its correct_fov_image handing back the prepared stacks, resident."""
    from imageanalysis3_amd import _lib as L
    from imageanalysis3_amd.correction_tools import chromatic as ch
    monkeypatch.setattr(ch, "correct_fov_image", R.prepared_correct_fov_image(upload=L.DeviceStack.upload))
    return ch


def test_find_chromatic_spot_pairs_matches_reference(prepared, golden, recorded, tmp_path):
    ch = prepared
    tol = recorded["tolerances"]["end_to_end_abs"]
    ca, ref = R.make_folders(str(tmp_path))
    infos = ch.find_chromatic_spot_pairs(os.path.join(ca, R.MOVIE_NAMES[0]), os.path.join(ref, R.MOVIE_NAMES[0]),
                                         R.CA_CHANNEL, R.REF_CHANNEL, R.BEAD_CHANNEL, correction_args=R.correction_args(),
                                         fitting_args=dict(R.FITTING_ARGS), rsq_th=R.RSQ_TH, save_temp=False, verbose=False)
    assert len(infos) == len(golden["pairs_rsquare"]) == recorded["conditions"]["b_pairs_below_above"][1]
    got = {k: np.array([i[k] for i in infos]) for k in ("ref_coord", "ca_coord", "rsquare", "slope", "intercept")}
    for k in ("ref_coord", "ca_coord"):              # the same pairs in the same order
        rel = np.abs(got[k].astype(np.float64) - golden["pairs_" + k]) / np.abs(golden["pairs_" + k])
        print(k, "largest relative difference:", rel.max())
        assert got[k].dtype == np.float32 and rel.max() < 1e-4, k
    for k in ("slope", "intercept", "rsquare"):
        diff = np.abs(got[k] - golden["pairs_" + k]).max()
        print(k, "largest difference:", diff, "allowed:", 2 * tol[k])
        assert diff <= 2 * tol[k], k
    for i in infos:
        assert {k: type(v).__name__ for k, v in i.items()} == recorded["types"]
        assert i["ref_im"].dtype == np.uint16 and i["ref_im"].shape == (9, 9, 9) == i["ca_im"].shape
        assert i["slope"].shape == (1,) and i["slope"].dtype == np.float64
        assert np.array_equal(i["drift"], golden["pairs_drift"])


@pytest.mark.parametrize("tag,orders", R.GENERATE_CASES)
def test_generate_chromatic_abbrevation_matches_reference(prepared, golden, recorded, tmp_path, tag, orders, capsys):
    ch = prepared
    tol = recorded["tolerances"]["end_to_end_abs"]
    ca, ref = R.make_folders(str(tmp_path))
    kw = dict(correction_args=R.correction_args(), fitting_args=dict(R.FITTING_ARGS), rsq_th=R.RSQ_TH,
              fitting_orders=orders, make_plots=False)
    pfs, consts = ch.Generate_chromatic_abbrevation(ca, ref, R.CA_CHANNEL, R.REF_CHANNEL, R.BEAD_CHANNEL, verbose=False, **kw)
    assert not [f for f in os.listdir(ca) if f.startswith("chromatic_correction")]      # silent: nothing saved
    assert len([f for f in os.listdir(ca) if f.startswith("chromatic_Conv")]) == 3
    pfs_v, consts_v = ch.Generate_chromatic_abbrevation(ca, ref, R.CA_CHANNEL, R.REF_CHANNEL, R.BEAD_CHANNEL, verbose=True, **kw)
    capsys.readouterr()
    base = os.path.join(ca, "chromatic_correction_750_647_20_96_96")
    assert np.array_equal(np.load(base + ".npy"), np.array(pfs_v)) and np.array_equal(np.array(pfs), np.array(pfs_v))
    with open(base + "_const.pkl", "rb") as f:
        cd = pickle.load(f)
    assert {k: type(v).__name__ for k, v in cd.items()} == recorded["const_types"]
    assert np.array_equal(cd["fitting_orders"], golden["gen_%s_orders" % tag])
    assert np.array_equal(cd["ref_center"], golden["gen_%s_ref_center" % tag])
    for a in range(3):
        diff = np.abs(consts[a] - golden["gen_%s_const%d" % (tag, a)]).max()
        print("constants of axis", a, "largest difference:", diff, "allowed:", 2 * tol["constants"])
        assert consts[a].shape == golden["gen_%s_const%d" % (tag, a)].shape and diff <= 2 * tol["constants"]
    diff = np.abs(np.array(cd["rsquares"]) - golden["gen_%s_rsquares" % tag]).max()
    print("rsquares largest difference:", diff, "allowed:", 2 * tol["rsquares"])
    assert diff <= 2 * tol["rsquares"]
    prof = np.array(pfs)
    assert prof.shape == (3,) + R.MOVIE_SHAPE and prof.dtype == np.float64
    diff = np.abs(prof[R.PROFILE_SAMPLE] - golden["gen_%s_profiles" % tag]).max()
    print("profiles largest difference:", diff, "allowed:", 2 * tol["profiles"])
    assert diff <= 2 * tol["profiles"]
    # the saved profile is the field of the saved constants
    for a in range(3):
        assert np.array_equal(prof[a], R.poly_field(R.MOVIE_SHAPE, cd["ref_center"], int(cd["fitting_orders"][a]), consts[a]))
    # load-if-exists: the files are read back, nothing is computed (the movies' temp files are gone)
    for f in os.listdir(ca):
        if f.startswith("chromatic_Conv"):
            os.remove(os.path.join(ca, f))
    pfs_l, consts_l = ch.Generate_chromatic_abbrevation(ca, ref, R.CA_CHANNEL, R.REF_CHANNEL, R.BEAD_CHANNEL, verbose=False,
                                                        **dict(kw, fitting_orders=3))
    assert np.array_equal(np.array(pfs_l), prof) and all(np.array_equal(x, y) for x, y in zip(consts_l, consts))
    assert not [f for f in os.listdir(ca) if f.startswith("chromatic_Conv")]
