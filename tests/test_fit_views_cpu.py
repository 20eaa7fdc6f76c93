"""CPU: the NumPy statement of the fitter's residual views (tests/harness/fit_views_ref.py) against the oracle, and the
host-side splitting of the packed device buffers into the reference's per-seed lists.

The statement is what the device implements (fit.hip): per voxel the image minus, in ascending seed order, every
reconstruction whose ball holds it.  After ``firstfit()`` that IS the reference's ``im_subtr`` (bit-equal); after
``repeatfit()`` the reference's ``im_add`` has been updated in place ball by ball — ``(im_add + rec_old) - rec_new`` —
and differs from the statement by the rounding order of those updates: measured 9.1e-13 absolute on ``clu_f32`` (4
sweeps), 1.05e-16 of the largest fitted height, 0 where no balls overlap.  The bar of 1e-12 of the largest fitted height
leaves four decades over that; a dropped term is of the order of a height."""
import numpy as np
import pytest

from harness import fit_views_ref as VR

FIXTURES = ["edge_f32", "clu_f32", "c1_u16"]
RADIUS = 5
oracle_fit = VR.oracle_fit


@pytest.mark.parametrize("name", FIXTURES)
def test_statement_is_the_oracles_im_subtr(name):
    im, seeds, first, f = oracle_fit(name)
    assert len(seeds) >= 8
    mine = VR.residual(im, seeds, first["ims_rec"], RADIUS)
    assert mine.dtype == np.float64 and mine.tobytes() == first["im_subtr"].tobytes()
    assert first["im_add"].tobytes() == first["im_subtr"].tobytes()
    assert f.im_subtr.tobytes() == first["im_subtr"].tobytes()      # repeatfit() leaves it alone
    count, owner = VR.coverage(im.shape, seeds, RADIUS)
    outside = count == 0
    assert outside.any() and np.array_equal(mine[outside], np.asarray(im, dtype=np.float64)[outside])
    assert (owner[~outside] >= 0).all()


@pytest.mark.parametrize("name", FIXTURES)
def test_statement_is_the_oracles_im_add_up_to_rounding_order(name):
    im, seeds, first, f = oracle_fit(name)
    mine = VR.residual(im, seeds, f.ims_rec, RADIUS)
    hmax = np.nanmax(np.array(f.ps, dtype=np.float64)[:, 0])
    diff = np.abs(mine - f.im_add).max()
    count, _ = VR.coverage(im.shape, seeds, RADIUS)
    print(name, "n_iter", f.n_iter, "max |statement - im_add| %.3g" % diff, "of hmax %.3g" % (diff / hmax),
          "voxels in > 1 ball", int((count > 1).sum()))
    assert diff <= 1e-12 * hmax
    if not (count > 1).any():
        assert diff == 0


def test_clustered_fixture_exercises_overlaps():
    im, seeds, first, f = oracle_fit("clu_f32")
    count, _ = VR.coverage(im.shape, seeds, RADIUS)
    assert (count > 1).sum() >= 1000 and count.max() >= 3
    assert f.n_iter >= 3 and all(f.success)
    assert tie_rule_differences(f, im.shape) >= 1


def tie_rule_differences(f, shape):
    """Seeds whose Voronoi cell under cKDTree's tie rule (the reference's) is not the lowest-index rule's."""
    n = 0
    for ic, c in enumerate(f.centers):
        X = VR.ball_voxels(c, RADIUS, shape)
        try:
            f.voronoi = "lowest_index"
            low = f._nearest_is_me(X, ic)
        finally:
            f.voronoi = "ckdtree"
        n += not np.array_equal(low, f._nearest_is_me(X, ic))
    return n


def test_owner_form_equals_seed_order_form():
    """The device writes every covered voxel once, from its owner's wave; the chain is the one the seed loop forms."""
    im, seeds, first, f = oracle_fit("clu_f32")
    assert VR.residual_by_owner(im, seeds, f.ims_rec, RADIUS).tobytes() == VR.residual(im, seeds, f.ims_rec, RADIUS).tobytes()
    im, seeds, first, f = oracle_fit("edge_f32")
    assert VR.residual_by_owner(im, seeds, f.ims_rec, RADIUS).tobytes() == VR.residual(im, seeds, f.ims_rec, RADIUS).tobytes()


def test_a_dropped_reconstruction_is_seen():
    im, seeds, first, f = oracle_fit("clu_f32")
    recs = list(f.ims_rec)
    recs[len(recs) // 2] = np.nan
    hmax = np.nanmax(np.array(f.ps, dtype=np.float64)[:, 0])
    assert np.abs(VR.residual(im, seeds, recs, RADIUS) - f.im_add).max() > 1e-3 * hmax


def test_split_packed_buffers():
    from imageanalysis3_amd.External.Fitting_v4 import split_voxel_sets, split_reconstructions
    nball = 6
    counts = np.array([3, 0, 6, 2], dtype=np.int32)
    zxy = np.arange(4 * nball * 3, dtype=np.int32).reshape(4, nball, 3)
    vals = np.arange(4 * nball, dtype=np.float64).reshape(4, nball) * 100 + 7
    centers = np.array([[1.0, 2.0, 3.0], [4.5, 5.0, 6.0], [7.0, 8.0, 9.0], [0.0, 0.0, 0.0]])
    for dt in (np.uint16, np.float32):
        g = split_voxel_sets(counts, zxy, vals, centers, dt)
        assert len(g) == 4
        for i, (im_, X, center) in enumerate(g):
            k = counts[i]
            assert im_.dtype == dt and im_.shape == (k,) and np.array_equal(im_, vals[i, :k].astype(dt))
            assert X.dtype == np.int64 and X.shape == (3, k) and np.array_equal(X, zxy[i, :k].T)
            assert isinstance(center, list) and center == list(centers[i])
    has = np.array([1, 0, 1, 0], dtype=np.uint8)
    recs = np.arange(4 * nball, dtype=np.float64).reshape(4, nball) / 3
    r = split_reconstructions(counts, has, recs)
    assert len(r) == 4
    assert r[0].dtype == np.float64 and np.array_equal(r[0], recs[0, :3]) and np.array_equal(r[2], recs[2])
    for k in (1, 3):   # the reference's placeholder: the scalar NaN, not an array
        assert isinstance(r[k], float) and np.isnan(r[k])
    r[0][0] = -1.0     # a copy, not a view of the download buffer
    assert recs[0, 0] == 0.0
    assert VR.has_rec(r[0]) and not VR.has_rec(r[1])
