"""GPU: the bleedthrough profile kernel ia3_bleedthrough_profile_dev (csrc/calib.hip) and the generator built on it
(correction_tools/bleedthrough.py).

The forward profile (invert=0) is compared bit for bit with the sequential statement of tests/harness/bleed_ref.py and,
within bleed_ref.tail_bound (n_cols * 2^-52 * sum |c_k m_k|, carried through the mean), with the matrices the reference
handed to np.linalg.inv (tests/golden/bleedthrough_tail.npz).  The inverse is compared with the exact rational inverse of
the device's own forward matrices, within 16 times the distance np.linalg.inv itself showed from it
(bleedthrough.json: tolerances.inverse_rel), and with the reference's inverse within that plus the forward bound
times ||A^-1||_inf^2.  find_bleedthrough_pairs and Generate_bleedthrough_correction are compared with the reference's
outputs within twice the change the reference itself shows when the fitted centres move by 1e-4 relative
(tolerances.end_to_end_abs).  Nothing here reads the reference tree."""
import json
import os
import pickle

import numpy as np
import pytest

from conftest import load_golden
from harness import bleed_ref as B
from harness import chrom_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return load_golden("bleedthrough.npz")


@pytest.fixture(scope="module")
def golden_tail():
    return load_golden("bleedthrough_tail.npz")


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(ROOT, "tests", "golden", "bleedthrough.json")) as f:
        return json.load(f)


def _profile(consts, present, order, center, shape, mean_z, invert, dtype=np.float64):
    from imageanalysis3_amd import _lib as L
    from imageanalysis3_amd.io_tools.load import DeviceBuffer
    n = consts.shape[0]
    out_shape = (n, n) + (tuple(shape[1:]) if mean_z else tuple(shape))
    buf = DeviceBuffer.adopt(L.bleedthrough_profile(consts, present, order, center, shape, mean_z=mean_z, invert=invert,
                                                    dtype=dtype), out_shape, dtype)
    try:
        return buf.download()
    finally:
        buf.free()


# ---- forward profile ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [0, 1])
def test_forward_profile_matches_statement_and_reference(golden_tail, s):
    """(3, 5, 7): odd rows, one pixel per thread; (12, 64, 96): 16 bytes per thread.  C = 3 with the direction 561 -> 750
    absent is the reference's case; C = 2 and 4 against the statement."""
    shape, center = B.TAIL_SHAPES[s], B.TAIL_CENTERS[s]
    for order in range(4):
        for n_ch, absent in ((3, ((0, 2),)), (2, ()), (4, ((3, 1), (0, 2)))):
            if n_ch != 3 and s == 1 and order in (0, 1):
                continue
            consts, present = B.tail_constants(n_ch, order, s, absent=absent)
            for mean_z in (True, False):
                f64 = _profile(consts, present, order, center, shape, mean_z, False)
                f32 = _profile(consts, present, order, center, shape, mean_z, False, np.float32)
                want = B.tail_forward(consts, present, order, center, shape, mean_z)
                assert f64.dtype == np.float64 and f64.shape == want.shape
                assert np.array_equal(f64, want), (order, n_ch, mean_z)
                assert f32.dtype == np.float32 and np.array_equal(f32, f64.astype(np.float32)), (order, n_ch, mean_z)
                for t, r in absent:
                    assert not f64[t, r].any()
                assert all(np.all(f64[k, k] == 1.0) for k in range(n_ch))
                if n_ch == 3:
                    ref = golden_tail["tail_s%d_o%d_%s_fwd" % (s, order, "2d" if mean_z else "3d")]
                    sample = B.tail_sample(s, mean_z)
                    bound = B.tail_bound(consts, present, order, center, shape, mean_z)[sample]
                    diff = np.abs(f64[sample] - ref)
                    print("order", order, "mean_z", mean_z, "largest difference from the reference's forward profile:",
                          diff.max(), "bound there:", bound[np.unravel_index(np.argmax(diff), diff.shape)])
                    assert np.all(diff <= bound), (order, mean_z)


@pytest.mark.parametrize("shape", [(1, 4, 8), (2, 3, 6), (2, 2, 1027), (1, 2, 1100)])
def test_forward_profile_store_paths(shape):
    """Rows of 16-byte multiples for both dtypes, for float64 only, for neither, and over several blocks."""
    center = (0.4, 1.3, shape[2] / 3.0)
    for n_ch, order in ((3, 3), (4, 2), (2, 1)):
        consts, present = B.tail_constants(n_ch, order, 0)
        consts = consts * (50.0 / max(shape)) ** 2          # keeps the polynomials small on the long rows too
        for mean_z in (True, False):
            f64 = _profile(consts, present, order, center, shape, mean_z, False)
            assert np.array_equal(f64, B.tail_forward(consts, present, order, center, shape, mean_z)), (n_ch, mean_z)
            f32 = _profile(consts, present, order, center, shape, mean_z, False, np.float32)
            assert np.array_equal(f32, f64.astype(np.float32)), (n_ch, mean_z)


# ---- inverse --------------------------------------------------------------------------------------------------------
def _inf_norm(M):
    return np.abs(M).sum(axis=2).max(axis=1)


@pytest.mark.parametrize("s", [0, 1])
def test_inverse_against_exact_arithmetic_and_reference(golden_tail, recorded, s):
    rec = recorded["tolerances"]["inverse_rel"]
    shape, center = B.TAIL_SHAPES[s], B.TAIL_CENTERS[s]
    worst = 0.0
    for order in range(4):
        consts, present = B.tail_constants(3, order, s, absent=((0, 2),))
        for mean_z in (True, False):
            sample = B.tail_sample(s, mean_z)
            fwd = _profile(consts, present, order, center, shape, mean_z, False)
            inv = _profile(consts, present, order, center, shape, mean_z, True)
            inv32 = _profile(consts, present, order, center, shape, mean_z, True, np.float32)
            assert np.array_equal(inv32, inv.astype(np.float32))
            A, Ai = B.matrices(fwd[sample]), B.matrices(inv[sample])
            step = 1 if s == 0 else 3                       # exact arithmetic on every third sampled matrix
            for a, ai in zip(A[::step], Ai[::step]):
                dist = B.inverse_distance(ai, a)
                worst = max(worst, dist)
                assert dist <= 16 * rec, (order, mean_z, dist, rec)
            key = "tail_s%d_o%d_%s" % (s, order, "2d" if mean_z else "3d")
            Gi = B.matrices(golden_tail[key + "_inv"])
            dA = B.matrices(B.tail_bound(consts, present, order, center, shape, mean_z)[sample])
            allowed = 16 * rec * np.abs(Gi).max(axis=(1, 2)) + _inf_norm(Gi) ** 2 * _inf_norm(dA)
            diff = np.abs(Ai - Gi).max(axis=(1, 2))
            assert np.all(diff <= allowed), (order, mean_z, float((diff / allowed).max()))
    print("largest distance from the exact inverse:", worst, "allowed:", 16 * rec)


@pytest.mark.parametrize("n_ch", [2, 4])
def test_inverse_of_two_and_four_channels(recorded, n_ch):
    rec = recorded["tolerances"]["inverse_rel"]
    shape, center = B.TAIL_SHAPES[0], B.TAIL_CENTERS[0]
    for order in (1, 3):
        consts, present = B.tail_constants(n_ch, order, 0)
        for mean_z in (True, False):
            fwd = _profile(consts, present, order, center, shape, mean_z, False)
            inv = _profile(consts, present, order, center, shape, mean_z, True)
            for a, ai in zip(B.matrices(fwd), B.matrices(inv)):
                dist = B.inverse_distance(ai, a)
                assert dist <= 16 * rec, (order, mean_z, dist)


def test_inverse_pivots_by_rows():
    """Matrices whose first pivot is not on the diagonal, and whose second is not either: the inverse times the matrix
    is the identity to rounding, against exact arithmetic."""
    shape, center = (1, 1, 2), (0.0, 0.0, 0.0)
    consts = np.zeros((3, 3, 1))
    consts[1, 0], consts[2, 0], consts[0, 1], consts[2, 1], consts[0, 2], consts[1, 2] = 4.0, -7.0, 0.5, 9.0, 0.25, 3.0
    fwd = _profile(consts, np.ones((3, 3)), 0, center, shape, True, False)
    inv = _profile(consts, np.ones((3, 3)), 0, center, shape, True, True)
    for a, ai in zip(B.matrices(fwd), B.matrices(inv)):
        assert np.array_equal(a, [[1, 0.5, 0.25], [4, 1, 3], [-7, 9, 1]])
        assert B.inverse_distance(ai, a) <= 16 * 2.0 ** -52 * np.linalg.cond(a, np.inf)


def test_singular_matrices_raise_and_are_counted():
    from imageanalysis3_amd import _lib as L
    shape, center = (3, 5, 7), (1.0, 2.0, 3.0)
    consts = np.zeros((2, 2, 4))
    consts[0, 1] = [1.0, 0.0, 0.0, 0.0]       # 1
    consts[1, 0] = [1.0, 0.0, 1.0, 0.0]       # 1 + (x - 2): [[1, 1], [1, 1]] on the row x = 2
    present = np.ones((2, 2))
    for mean_z, count in ((True, 7), (False, 21)):
        fwd = _profile(consts, present, 1, center, shape, mean_z, False)
        assert int(np.sum((fwd[0, 1] == 1.0) & (fwd[1, 0] == 1.0))) == count
        with pytest.raises(np.linalg.LinAlgError) as e:
            L.bleedthrough_profile(consts, present, 1, center, shape, mean_z=mean_z, invert=True)
        assert str(e.value) == "Singular matrix" and e.value.n_singular == count


def test_profile_arguments():
    from imageanalysis3_amd import _lib as L
    c3 = np.zeros((3, 3, 4))
    with pytest.raises(NotImplementedError):
        L.bleedthrough_profile(np.zeros((5, 5, 4)), np.ones((5, 5)), 1, np.zeros(3), (2, 2, 2))
    with pytest.raises(NotImplementedError):
        L.bleedthrough_profile(np.zeros((3, 3, 35)), np.ones((3, 3)), 4, np.zeros(3), (2, 2, 2))
    with pytest.raises(ValueError):
        L.bleedthrough_profile(np.zeros((3, 3, 5)), np.ones((3, 3)), 1, np.zeros(3), (2, 2, 2))
    with pytest.raises(ValueError):
        L.bleedthrough_profile(c3, np.ones((3, 2)), 1, np.zeros(3), (2, 2, 2))
    with pytest.raises(ValueError):
        L.bleedthrough_profile(c3, np.ones((3, 3)), 1, np.zeros(3), (2, 0, 2))
    with pytest.raises(ValueError):
        L.bleedthrough_profile(np.zeros((1, 1, 4)), np.ones((1, 1)), 1, np.zeros(3), (2, 2, 2))
    with pytest.raises(TypeError):
        L.bleedthrough_profile(c3, np.ones((3, 3)), 1, np.zeros(3), (2, 2, 2), dtype=np.float16)


# ---- the generator --------------------------------------------------------------------------------------------------
@pytest.fixture()
def prepared(monkeypatch):
    """correction_tools/bleedthrough.py with its correct_fov_image handing back the prepared stacks, resident."""
    from imageanalysis3_amd import _lib as L
    from imageanalysis3_amd.correction_tools import bleedthrough as bl
    monkeypatch.setattr(bl, "correct_fov_image", B.prepared_correct_fov_image(upload=L.DeviceStack.upload))
    return bl


def _fitting_args(bl):
    return dict(bl._bleedthrough_default_fitting_args, **B.FITTING_ARGS)


def test_find_bleedthrough_pairs_matches_reference(prepared, golden, recorded, tmp_path):
    bl = prepared
    tol = recorded["tolerances"]["end_to_end_abs"]
    folders = B.make_folders(str(tmp_path))
    name, c = B.USED_NAMES[0], '750'
    got = bl.find_bleedthrough_pairs(os.path.join(folders[0], name), c, list(B.CHANNELS), B.correction_args(),
                                     _fitting_args(bl), -np.inf, 9, -np.inf, False, False, None, True, False)
    assert sorted(got) == ["750_to_561", "750_to_647"]
    assert not [f for f in os.listdir(folders[0]) if f.endswith(".pkl")]
    stacks = B.movie(c, name)
    same_box = 0
    for t in ('647', '561'):
        pre = "pairs_%d_%s_to_%s_" % (B.movie_number(name), c, t)
        infos = got["%s_to_%s" % (c, t)]
        assert len(infos) == len(golden[pre + "rsquare"])
        coord = np.array([i['coord'] for i in infos])
        rel = np.abs(coord.astype(np.float64) - golden[pre + "coord"]) / np.abs(golden[pre + "coord"])
        print(t, "centres: largest relative difference", rel.max())
        assert coord.dtype == np.float32 and rel.max() < 1e-4                    # the same pairs in the same order
        kept = np.array([bl.check_bleedthrough_info(i, B.RSQ_TH, B.INTENSITY_TH, True) for i in infos])
        assert np.array_equal(kept, golden[pre + "kept"])
        for q in ("slope", "intercept", "rsquare"):
            diff = np.abs(np.array([i[q] for i in infos]) - golden[pre + q])[kept].max()
            print(t, q, "largest difference:", diff, "allowed:", 2 * tol[q])
            assert diff <= 2 * tol[q], (t, q)
        for k, i in enumerate(infos):
            assert {key: type(v).__name__ for key, v in i.items()} == recorded["types"]
            assert i['ref_im'].dtype == np.uint16 and i['ref_im'].shape == (9, 9, 9) == i['bleed_im'].shape
            assert i['spot'].dtype == np.float32 and i['spot'].shape == (11,) and np.array_equal(i['coord'], i['spot'][1:4])
            assert i['slope'].dtype == np.float64 and i['file'] == os.path.join(folders[0], name)
            # wherever both centres give the same box (stated on the host), the box is the reference's
            for im, key in ((stacks[c], "ref_im"), (stacks[t], "bleed_im")):
                if np.array_equal(R.crop_neighboring_area(im, golden[pre + "coord"][k], 9),
                                  R.crop_neighboring_area(im, i['coord'], 9)):
                    same_box += 1
                    assert np.array_equal(i[key], golden[pre + key][k]), (t, k, key)
    print("boxes compared with the reference's:", same_box)
    assert same_box >= 32


def _run_generate(bl, folders, order, g2d, **kw):
    return bl.Generate_bleedthrough_correction(folders, **dict(B.generate_kwargs(order, g2d), **kw))


@pytest.mark.parametrize("tag,order,g2d", B.GENERATE_CASES)
def test_generate_bleedthrough_correction_matches_reference(prepared, golden, recorded, tmp_path, tag, order, g2d):
    bl = prepared
    tol = recorded["tolerances"]["end_to_end_abs"]
    files = recorded["files"][tag]
    folders = B.make_folders(str(tmp_path))
    prof = _run_generate(bl, folders, order, g2d)
    assert list(prof.shape) == files["returned_shape"] and str(prof.dtype) == files["dtype"]
    made = [f for f in os.listdir(folders[0]) if f.endswith(".npy")]
    assert made == [files["name"]] == [B.profile_name(g2d)]
    saved = np.load(os.path.join(folders[0], made[0]))
    assert list(saved.shape) == files["saved_shape"] and np.array_equal(saved.reshape(prof.shape), prof)
    for folder, c in zip(folders, B.CHANNELS):             # temp files of the four movies after start_fov, both targets
        assert sorted(f for f in os.listdir(folder) if f.endswith(".pkl")) == \
            sorted(B.temp_name(n, c, t) for n in B.USED_NAMES for t in B.CHANNELS if t != c)
    sample = B.PROFILE_SAMPLE_2D if g2d else B.PROFILE_SAMPLE_3D
    diff = np.abs(prof[sample] - golden["gen_%s_profile" % tag]).max()
    print("profile: largest difference", diff, "allowed:", 2 * tol["profile"])
    assert diff <= 2 * tol["profile"]
    # the temp files hold the pairs: from them the mixing matrices before inversion, and the same profile again
    dicts = [bl.find_bleedthrough_pairs(os.path.join(folder, n), c, list(B.CHANNELS), B.correction_args(), _fitting_args(bl),
                                        B.INTENSITY_TH, 9, B.RSQ_TH, True, True, None, False, False)
             for n in B.USED_NAMES for folder, c in zip(folders, B.CHANNELS)]
    kw = dict(single_im_size=B.MOVIE_SHAPE, fitting_order=order, generate_2d=g2d,
              interpolate_args={'min_num_spots': B.MIN_NUM_SPOTS}, verbose=False, dtype=np.float64)
    fwd_buf = bl.bleedthrough_profile_from_pairs(dicts, B.CHANNELS, invert=False, **kw)
    inv_buf = bl.bleedthrough_profile_from_pairs(dicts, B.CHANNELS, **kw)
    try:
        fwd, inv = fwd_buf.download(), inv_buf.download()
    finally:
        fwd_buf.free()
        inv_buf.free()
    assert np.array_equal(inv, prof)
    assert not fwd[0, 2].any()                               # 561 -> 750: the zero profile, exactly
    assert all(np.all(fwd[k, k] == 1.0) for k in range(3))
    consts, present, fits = bl._profile_arguments(dicts, B.CHANNELS, order, {'min_num_spots': B.MIN_NUM_SPOTS}, False)
    assert present.tolist() == [[0, 1, 0], [1, 0, 1], [1, 1, 0]] and fits[('561', '750')] is None
    assert np.array_equal(fwd, B.tail_forward(consts, present, order, np.array(B.MOVIE_SHAPE) / 2, B.MOVIE_SHAPE, g2d))
    # load-if-exists: the file is read back as it is (C * C first), nothing is computed
    for folder in folders:
        for f in os.listdir(folder):
            if f.endswith(".pkl"):
                os.remove(os.path.join(folder, f))
    loaded = _run_generate(bl, folders, 3, g2d)
    assert list(loaded.shape) == files["loaded_shape"] and np.array_equal(loaded, saved)
    assert not [f for folder in folders for f in os.listdir(folder) if f.endswith(".pkl")]


def test_generate_draws_its_figures_from_z_means(prepared, tmp_path):
    """make_plots: two figures per direction that passes, saved beside the profile; the profile is the same."""
    pytest.importorskip("matplotlib")
    bl = prepared
    folders = B.make_folders(str(tmp_path))
    prof = _run_generate(bl, folders, 1, True, make_plots=True, save_plots=True)
    pngs = sorted(f for f in os.listdir(folders[0]) if f.endswith(".png"))
    want = sorted("bleedthrough_profile_%s_to_%s_%s.png" % (r, t, q) for (r, t), sl in B.SLOPES.items() if sl is not None
                  for q in ("slope", "intercept"))
    assert pngs == want
    quiet = _run_generate(bl, folders, 1, True, overwrite_profile=True)
    assert np.array_equal(prof, quiet)


def test_partial_temp_files_are_kept_and_appended_to(prepared, golden, recorded, tmp_path):
    bl = prepared
    part = recorded["partial"]
    folders = B.make_folders(str(tmp_path))
    name, c = part["movie"], part["channel"]
    folder = folders[B.CHANNELS.index(c)]
    args = (os.path.join(folder, name), c, list(B.CHANNELS), B.correction_args(), _fitting_args(bl), B.INTENSITY_TH, 9,
            B.RSQ_TH, True, True, None)
    first = bl.find_bleedthrough_pairs(*args, True, False)
    present_file = os.path.join(folder, B.temp_name(name, c, '750'))
    missing_file = os.path.join(folder, B.temp_name(name, c, part["missing"]))
    with open(present_file, 'rb') as f:
        assert len(pickle.load(f)) == part["stored_before"]
    os.remove(missing_file)
    got = bl.find_bleedthrough_pairs(*args, False, False)
    assert {k: len(v) for k, v in got.items()} == part["returned"]
    with open(present_file, 'rb') as f:
        assert len(pickle.load(f)) == part["stored_after"]
    assert os.path.isfile(missing_file)
    n = len(first["647_to_750"])
    for key in ("647_to_750", "647_to_561"):
        coord = np.array([i['coord'] for i in got[key]], dtype=np.float64)
        assert np.abs(coord - golden["partial_%s_coord" % key]).max() < 1e-4 * 96
    assert all(np.array_equal(a['coord'], b['coord']) for a, b in zip(got["647_to_750"][:n], got["647_to_750"][n:]))
    again = bl.find_bleedthrough_pairs(*args, False, False)      # both files there: loaded, nothing appended
    assert {k: len(v) for k, v in again.items()} == part["returned"]


def test_round_trip_from_pairs_to_corrected_images(prepared, recorded, tmp_path):
    """Pairs -> resident float32 profile -> correct_fov_image(bleed_profile=...) on a three-channel movie mixed with the
    planted slopes: the unmixed channels come back within one grey level plus the slope tolerance times the channel
    maximum, the slope tolerance being the one the other generator tests use: twice the recorded change of (d).  ref_center = 0: the reference fits the polynomial on the coordinates as they are and evaluates
    it at pixel coordinates minus ref_center (bleedthrough.py:298, :314-316), so only then does the profile describe the
    mixing at the pixel it is stored at; fitting_order 1 is the planted model."""
    from imageanalysis3_amd import synth
    from imageanalysis3_amd.io_tools.load import correct_fov_image, DeviceBuffer
    bl = prepared
    tol = recorded["tolerances"]["end_to_end_abs"]["slope"]
    folders = B.make_folders(str(tmp_path))
    dicts = [bl.find_bleedthrough_pairs(os.path.join(folder, n), c, list(B.CHANNELS), B.correction_args(), _fitting_args(bl),
                                        B.INTENSITY_TH, 9, B.RSQ_TH, True, False, None, True, False)
             for n in B.USED_NAMES for folder, c in zip(folders, B.CHANNELS)]
    buf = bl.bleedthrough_profile_from_pairs(dicts, B.CHANNELS, B.MOVIE_SHAPE, fitting_order=1,
                                             interpolate_args={'min_num_spots': B.MIN_NUM_SPOTS}, ref_center=np.zeros(3),
                                             verbose=False)
    try:
        assert isinstance(buf, DeviceBuffer) and buf.shape == (3, 3) + B.MOVIE_SHAPE[1:] and buf.dtype == np.float32
        pure = [synth.make_fov(B.MOVIE_SHAPE, 12, 7900 + k, dtype=np.uint16, margin=(3, 8, 8), h_range=B.H_RANGE)[0].astype(np.float64)
                for k in range(3)]
        x = np.arange(B.MOVIE_SHAPE[1], dtype=np.float64)[None, :, None]
        mixed = []
        for t, tar in enumerate(B.CHANNELS):
            im = pure[t].copy()
            for r, ref in enumerate(B.CHANNELS):
                sl = None if r == t else B.planted_slope(ref, tar, x)
                if sl is not None:
                    im = im + sl * pure[r]
            mixed.append(synth.quantise(im, np.uint16))
        chs = B.CHANNELS + ['488']
        raw = np.zeros((4 * B.MOVIE_SHAPE[0],) + B.MOVIE_SHAPE[1:], np.uint16)
        for k in range(3):
            raw[k::4] = mixed[k]
        out = correct_fov_image(raw, B.CHANNELS, single_im_size=list(B.MOVIE_SHAPE), all_channels=chs, num_buffer_frames=0,
                                num_empty_frames=0, corr_channels=B.CHANNELS, warp_image=False, hot_pixel_corr=False,
                                z_shift_corr=False, illumination_corr=False, chromatic_corr=False, bleed_corr=True,
                                bleed_profile=buf, verbose=False)[0]
        top = max(float(p.max()) for p in pure)
        for k in range(3):
            err = np.abs(out[k].astype(np.float64) - pure[k]).max()
            print(B.CHANNELS[k], "largest error:", err, "allowed:", 1.0 + 2 * tol * top,
                  "uncorrected:", np.abs(mixed[k].astype(np.float64) - pure[k]).max())
            assert err <= 1.0 + 2 * tol * top
    finally:
        buf.free()
