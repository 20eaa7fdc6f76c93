"""GPU: the views of a fit — ``gparms``, ``ims_rec``, ``im_subtr``, ``im_add`` and ``residual_stack()`` of
``External.Fitting_v4.iter_fit_seed_points`` (fit.hip, "Views of a finished fit") — against the oracle (oracle/
np_oracle.py, cKDTree's tie rule), against the NumPy statement of the residual (tests/harness/fit_views_ref.py, held to
the oracle by tests/test_fit_views_cpu.py) and against the class's own closed-form model on the host.

Exact (no tolerance): voxel sets and their values, counts, lengths, dtypes; the residual images against the statement fed
with the device's own ``ims_rec``; ``im_subtr`` before and after ``repeatfit()``; the float32 stack against the rounded
float64 image; two runs; the seed-list scan against the neighbour lists.

Measured on the MI355X (every seed of ``edge_f32``, ``clu_f32``, ``c1_u16``; the tests print the figures):

* ``ims_rec`` against ``GaussianFit.calc_f`` in float64 at the device's own records (the two differ in ``exp`` and in the
  square roots and divisions of the geometry), largest |device - host| / max(host) of a seed: edge_f32 6.52e-16 after the
  first fit and 1.29e-15 after the sweeps, clu_f32 1.38e-15 / 1.55e-15, c1_u16 1.79e-15 / 1.23e-15 (c1_f32, first fit:
  1.57e-15).  MEASURED_REC_MODEL is the largest, the bar four times that: 7.2e-15, some thirty float64 units in the last
  place.
* against the oracle, ``ims_rec`` over the seed's fitted height after the first fit / after the sweeps, ``im_subtr`` and
  ``im_add`` over the largest fitted height: edge_f32 2.48e-15 / 2.30e-15 / 1.38e-15 / 1.54e-15, clu_f32 4.39e-15 /
  4.82e-15 / 1.69e-15 / 3.21e-15, c1_u16 4.60e-15 / 4.83e-15 / 3.04e-15 / 3.73e-15.  MEASURED_ORACLE holds the largest per
  fixture; the bar is four times the largest of them, 1.9e-14 (never above the project's 1e-4).  The fits themselves run
  the same operations in the same order on both sides, which is why the records agree this closely.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import build_case, build_legacy, load_golden
from harness import fit_views_ref as VR
from imageanalysis3_amd._lib import IA3_TUNE_FIT_NBLIST

pytestmark = pytest.mark.gpu

FIXTURES = ["edge_f32", "clu_f32", "c1_u16"]
RADIUS = 5

# largest relative difference between ims_rec and the host model at the same records, over all seeds of the fixtures
MEASURED_REC_MODEL = 1.79e-15
REC_MODEL_BAR = 4 * MEASURED_REC_MODEL
# largest normalised difference to the oracle per fixture (over ims_rec first / final, im_subtr, im_add)
MEASURED_ORACLE = {"edge_f32": 2.48e-15, "clu_f32": 4.82e-15, "c1_u16": 4.83e-15}
ORACLE_BAR = min(1e-4, 4 * max(MEASURED_ORACLE.values()))


def _fitter(im, seeds, cls=None, radius=RADIUS, **kw):
    from imageanalysis3_amd.External.Fitting_v4 import iter_fit_seed_points
    return (cls or iter_fit_seed_points)(im, np.asarray(seeds).T, radius_fit=radius, **kw)


def _host_model(x11, seed, X, min_w=0.5, max_w=4.):
    """``GaussianFit.get_im()`` (the class's float64 ``calc_f``) on the voxels X at the record x11 = (p_, delta_center)."""
    from imageanalysis3_amd.External.Fitting_v4 import GaussianFit
    g = GaussianFit(np.ones(X.shape[1], dtype=np.float32), X, center=list(seed), delta_center=float(x11[10]),
                    min_w=min_w, max_w=max_w)
    g.x, g.y, g.z = X                                              # as firstfit() does before get_im() (:630)
    g.calc_f(np.array(x11[:10], dtype=np.float64))
    return g, np.asarray(g.f0, dtype=np.float64)


def _model_gap(f, which, seeds, shape):
    """Largest |ims_rec - host model| / max(host model) over the seeds with a reconstruction, and the records."""
    cnt, has, recs, x11 = f._records(which)
    worst = 0.0
    for i, c in enumerate(seeds):
        if not has[i]:
            continue
        X = VR.ball_voxels(c, RADIUS, shape)
        _, want = _host_model(x11[i], c, X)
        got = recs[i, :cnt[i]]
        assert len(got) == len(want)
        worst = max(worst, float(np.abs(got - want).max() / want.max()))
    return worst, x11, has


# ---- 1 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_voxel_sets_equal_oracle(name):
    im, seeds, first, fo = VR.oracle_fit(name)
    f = _fitter(im, seeds)
    for attr in ("gparms", "ims_rec", "im_subtr", "im_add"):
        with pytest.raises(AttributeError):
            getattr(f, attr)
    f.firstfit()
    nvox = np.array(f.nvox)
    g = f.gparms
    assert len(g) == len(seeds) == len(fo.gparms) and len(f.ims_rec) == len(seeds)
    for i, ((im_, X, center), (oim, oX, ocenter)) in enumerate(zip(g, fo.gparms)):
        assert X.dtype == np.int64 and X.shape == (3, nvox[i]) and np.array_equal(X, oX), i
        assert im_.dtype == im.dtype and im_.tobytes() == np.ascontiguousarray(oim).tobytes(), i
        assert isinstance(center, list) and center == list(seeds[i]) == list(ocenter)
        ro, rd = first["ims_rec"][i], f.ims_rec[i]
        assert VR.has_rec(rd) == VR.has_rec(ro) == bool(f.success[i])
        if VR.has_rec(rd):
            assert rd.dtype == np.float64 and rd.shape == ro.shape == (VR.ball_voxels(seeds[i], RADIUS, im.shape).shape[1],)
    assert f.gparms is g                                           # rendered once, cached
    for a in (f.im_subtr, f.im_add):
        assert a.dtype == np.float64 and a.shape == im.shape
    if name == "clu_f32":   # the cells are the reference's, not the lowest-index rule's
        diff = sum(not np.array_equal(np.asarray(a[1]), b[1]) for a, b in zip(
            _lowest_index_cells(fo, im.shape), g))
        assert diff >= 1


@pytest.mark.parametrize("radius", [2, 3, 4])
def test_voxel_sets_equal_oracle_partly_filled_slot(radius):
    """test_voxel_sets_equal_oracle's geometry at the radii whose ball ends inside a slot (30, 120 and 254 voxels: slot 0,
    slot 1 partly filled, slot 3 filled up to two lanes) on the clustered fixture, where seeds lie within 2r of each other
    at every one of them (the oracle alone cuts 1 and 10 cells at radius 2 and 3): voxel sets, their values and the first fit's voxel counts, exactly.  No fitted row is compared."""
    name = "clu_f32"
    im, seeds, _, fo = VR.oracle_fit(name, radius)
    whole = [VR.ball_voxels(c, radius, im.shape).shape[1] for c in seeds]
    assert len(VR.ball_offsets(radius)[0]) % 64 != 0
    assert sum(oX.shape[1] < n for (_, oX, _), n in zip(fo.gparms, whole)) >= 1     # the neighbour path is exercised
    f = _fitter(im, seeds, radius=radius)
    f.firstfit()
    nvox = np.array(f.nvox)
    g = f.gparms
    assert len(g) == len(seeds) == len(fo.gparms) == len(nvox)
    for i, ((im_, X, _), (oim, oX, _)) in enumerate(zip(g, fo.gparms)):
        assert nvox[i] == oX.shape[1], i
        assert X.dtype == np.int64 and X.shape == (3, nvox[i]) and np.array_equal(X, oX), i
        assert im_.dtype == im.dtype and im_.tobytes() == np.ascontiguousarray(oim).tobytes(), i


def _lowest_index_cells(fo, shape):
    out = []
    for ic, c in enumerate(fo.centers):
        X = VR.ball_voxels(c, RADIUS, shape)
        try:
            fo.voronoi = "lowest_index"
            keep = fo._nearest_is_me(X, ic)
        finally:
            fo.voronoi = "ckdtree"
        out.append([None, X[:, keep]])
    return out


# ---- 2 -----------------------------------------------------------------------------------------------------------------
def _identities(im, seeds, make, repeat=True):
    """Test 2's identities on one input; returns the bytes of everything rendered (for the run-to-run comparison)."""
    count, _ = VR.coverage(im.shape, seeds, RADIUS)
    im64 = np.asarray(im, dtype=np.float64)
    f = make()
    f.firstfit()
    blob = []
    subtr0 = None
    for stage in ("first", "final") if repeat else ("first",):
        if stage == "final":
            f.repeatfit()
        recs = f.ims_rec
        for w in ("subtr", "add"):
            vol = getattr(f, "im_" + w)
            if stage == "first" or w == "add":
                want = VR.residual(im, seeds, recs, RADIUS)
            else:
                want = subtr0                                    # the snapshot: repeatfit() does not touch im_subtr
            assert vol.dtype == np.float64 and vol.tobytes() == want.tobytes(), (stage, w)
            assert np.array_equal(vol[count == 0], im64[count == 0])
            with f.residual_stack(w) as st:
                assert st.dtype == np.float32 and st.shape == im.shape
                assert st.download().tobytes() == vol.astype(np.float32).tobytes(), (stage, w)
            blob.append(vol.tobytes())
        if stage == "first":
            subtr0 = f.im_subtr
        blob.extend(r.tobytes() for r in recs if VR.has_rec(r))
        blob.extend(g[0].tobytes() + g[1].tobytes() for g in f.gparms)
    f.release()
    return blob


@pytest.mark.parametrize("name", FIXTURES)
def test_residuals_are_the_statement_exactly(name):
    im, seeds, first, fo = VR.oracle_fit(name)
    a = _identities(im, seeds, lambda: _fitter(im, seeds))
    b = _identities(im, seeds, lambda: _fitter(im, seeds))
    assert a == b                                                  # two fitters, identical bytes
    if name == "clu_f32":
        from imageanalysis3_amd import _lib as L
        count, _ = VR.coverage(im.shape, seeds, RADIUS)
        assert (count > 1).sum() >= 1000 and count.max() >= 3 and fo.n_iter >= 3
        d2 = ((seeds[:, None, :] - seeds[None, :, :]) ** 2).sum(-1)
        assert ((d2 <= (2.0 * RADIUS) ** 2).sum(1) - 1).max() > 2      # some seed has more neighbours than the list takes
        try:
            L.check(L.lib().ia3_set_tuning(C.c_int(IA3_TUNE_FIT_NBLIST), C.c_int(2)))
            c = _identities(im, seeds, lambda: _fitter(im, seeds))
        finally:
            L.check(L.lib().ia3_set_tuning(C.c_int(IA3_TUNE_FIT_NBLIST), C.c_int(64)))
        assert c == a                                              # the seed-list scan: the same bytes


# ---- 3 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_reconstructions_against_host_model(name):
    im, seeds, first, fo = VR.oracle_fit(name)
    f = _fitter(im, seeds)
    f.firstfit()
    gap_first, _, _ = _model_gap(f, 0, seeds, im.shape)
    f.repeatfit()
    gap_snap, _, _ = _model_gap(f, 0, seeds, im.shape)
    gap_final, _, has = _model_gap(f, 1, seeds, im.shape)
    print(name, "ims_rec vs host model: first %.3g  snapshot %.3g  final %.3g  (bar %.3g)"
          % (gap_first, gap_snap, gap_final, REC_MODEL_BAR))
    assert has.all() == all(VR.has_rec(r) for r in f.ims_rec)
    assert gap_first == gap_snap                                   # the snapshot is what the first fit left
    assert max(gap_first, gap_final) <= REC_MODEL_BAR


# ---- 4 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_views_against_oracle(name):
    im, seeds, first, fo = VR.oracle_fit(name)
    f = _fitter(im, seeds)
    f.firstfit()
    assert list(f.success) == list(first["success"])

    def rec_gap(mine, theirs, heights):
        worst = 0.0
        for a, b, h in zip(mine, theirs, heights):
            assert VR.has_rec(a) == VR.has_rec(b)
            if VR.has_rec(a):
                worst = max(worst, float(np.abs(a - b).max() / h))
        return worst
    g_first = rec_gap(f.ims_rec, first["ims_rec"], first["ps"][:, 0])
    hmax1 = np.nanmax(first["ps"][:, 0])
    g_subtr = float(np.abs(f.im_subtr - first["im_subtr"]).max() / hmax1)
    f.repeatfit()
    assert f.n_iter == fo.n_iter and list(f.success) == list(fo.success)
    ps = np.array(fo.ps, dtype=np.float64)
    g_final = rec_gap(f.ims_rec, fo.ims_rec, ps[:, 0])
    hmax2 = np.nanmax(ps[:, 0])
    g_add = float(np.abs(f.im_add - fo.im_add).max() / hmax2)
    g_subtr2 = float(np.abs(f.im_subtr - fo.im_subtr).max() / hmax1)
    print(name, "against the oracle: ims_rec first %.3g final %.3g  im_subtr %.3g  im_add %.3g  (bar %.3g)"
          % (g_first, g_final, g_subtr, g_add, ORACLE_BAR))
    assert g_subtr2 == g_subtr
    assert max(g_first, g_final, g_subtr, g_add) <= ORACLE_BAR


# ---- 5 -----------------------------------------------------------------------------------------------------------------
def test_no_reconstruction():
    import np_oracle as O
    im = build_case("edge_f32")
    seeds = O.get_seeds(im, th_seed=600)
    fo = O.iter_fit_seed_points(im, seeds.T, radius_fit=1)
    fo.firstfit()
    assert len(seeds) >= 8 and not any(fo.success) and all(len(g[0]) <= 4 for g in fo.gparms)
    from imageanalysis3_amd.External.Fitting_v4 import iter_fit_seed_points
    f = iter_fit_seed_points(im, seeds.T, radius_fit=1)
    f.firstfit()
    im64 = np.asarray(im, dtype=np.float64)
    for stage in range(2):
        assert not any(f.success)
        assert all(isinstance(r, float) and np.isnan(r) for r in f.ims_rec)
        for (im_, X, c), (oim, oX, oc) in zip(f.gparms, fo.gparms):
            assert np.array_equal(X, oX) and im_.tobytes() == np.ascontiguousarray(oim).tobytes() and X.shape[1] <= 4
        assert f.im_subtr.tobytes() == im64.tobytes() and f.im_add.tobytes() == im64.tobytes()
        with f.residual_stack("add") as st:
            assert st.download().tobytes() == im.astype(np.float32).tobytes()
        if stage == 0:
            f.repeatfit()
            fo.repeatfit()
            assert fo.im_add.tobytes() == im64.tobytes()


# ---- 6 -----------------------------------------------------------------------------------------------------------------
def test_isolated_seeds_first_fit_records():
    """After firstfit() alone, on isolated seeds (which ia3_fit_run would give their sweep 1 in the same wave): the
    records behind ims_rec are the FIRST fit's — their delta_center is min_delta_center, their natural parameters are
    f.ps (float32: one unit in the last place for the host's exp / sqrt against the device's) — and ims_rec is the host
    model at them to test 3's bar."""
    import np_oracle as O
    im = build_case("c1_f32")
    seeds = O.get_seeds(im, th_seed=600)
    d2 = ((seeds[:, None, :] - seeds[None, :, :]) ** 2).sum(-1) + np.eye(len(seeds)) * 1e9
    assert len(seeds) >= 40 and d2.min() > (2.0 * RADIUS) ** 2           # no ball meets another
    f = _fitter(im, seeds)
    f.firstfit()
    assert all(f.success)
    gap, x11, has = _model_gap(f, 1, seeds, im.shape)
    gap0, x11_0, _ = _model_gap(f, 0, seeds, im.shape)
    print("c1_f32 first-fit ims_rec vs host model %.3g (bar %.3g)" % (gap, REC_MODEL_BAR))
    assert has.all() and x11.tobytes() == x11_0.tobytes() and gap == gap0
    assert (x11[:, 10] == f.min_delta_center).all() and f.min_delta_center != f.max_delta_center
    ps = np.array(f.ps)
    for i, c in enumerate(seeds):
        g, _ = _host_model(x11[i], c, VR.ball_voxels(c, RADIUS, im.shape))
        nat = g.to_natural_paramaters(np.array(x11[i, :10]))
        np.testing.assert_allclose(nat[:10], ps[i, :10], rtol=2.0 ** -23, atol=1e-12)
    assert gap <= REC_MODEL_BAR
    for r, c in zip(f.ims_rec, seeds):
        assert r.shape == (VR.ball_voxels(c, RADIUS, im.shape).shape[1],)


def test_records_carry_the_delta_center_of_their_fit():
    """x11[:, 10] of the first-fit records is the caller's min_delta_center, of the current records after repeatfit() the
    caller's max_delta_center — off the defaults, the first larger than the second — and each reconstruction is the host
    model at its own record and delta to test 3's bar."""
    import np_oracle as O
    im = build_case("clu_f32")
    seeds = O.get_seeds(im, th_seed=600)
    f = _fitter(im, seeds, min_delta_center=1.75, max_delta_center=0.5)
    f.firstfit()
    gap0, x11_0, has0 = _model_gap(f, 0, seeds, im.shape)
    has0 = has0.astype(bool)
    assert has0.any() and (x11_0[has0, 10] == 1.75).all()
    f.repeatfit()
    gap1, x11_1, has1 = _model_gap(f, 1, seeds, im.shape)
    _, x11_k, has_k = _model_gap(f, 0, seeds, im.shape)
    has1, has_k = has1.astype(bool), has_k.astype(bool)
    print("clu_f32 deltas 1.75 / 0.5: ims_rec vs host model first %.3g final %.3g (bar %.3g)" % (gap0, gap1, REC_MODEL_BAR))
    assert has1.any() and (x11_1[has1, 10] == 0.5).all()
    assert x11_k.tobytes() == x11_0.tobytes() and np.array_equal(has_k, has0)     # the first fit's records are kept
    assert max(gap0, gap1) <= REC_MODEL_BAR
    ps = np.array(f.ps)
    assert (np.abs(ps[has1, 1:4] - seeds[has1]).max(axis=1) <= 0.5 + 1e-6).all()


# ---- 7 -----------------------------------------------------------------------------------------------------------------
def test_second_pass_on_the_device():
    from imageanalysis3_amd import _lib as L
    from imageanalysis3_amd.spot_tools.fitting import get_seeds
    im, seeds, first, fo = VR.oracle_fit("clu_f32")
    d2 = ((seeds[:, None, :] - seeds[None, :, :]) ** 2).sum(-1) + np.eye(len(seeds)) * 1e9
    k = int(np.argmax(d2.min(1) <= (2.0 * RADIUS) ** 2))         # the brightest seed whose ball meets another one
    assert d2[k].min() <= (2.0 * RADIUS) ** 2
    rest = np.delete(seeds, k, axis=0)
    f = _fitter(im, rest)
    f.firstfit()
    f.repeatfit()
    with f.residual_stack("add") as st:
        on_dev = get_seeds(st, th_seed=600, return_h=True)
        arr = st.download()
    assert arr.dtype == np.float32 and arr.tobytes() == f.im_add.astype(np.float32).tobytes()
    with L.DeviceStack.upload(arr) as again:
        assert get_seeds(again, th_seed=600, return_h=True).tobytes() == on_dev.tobytes()
    assert get_seeds(arr, th_seed=600, return_h=True).tobytes() == on_dev.tobytes()
    # the blob whose seed was withheld is what the residual still holds: its maximum is a seed of the second pass
    off = np.abs(on_dev[:, :3] - seeds[k]).max(1)
    print("withheld seed", k, seeds[k], "nearest residual seed at Chebyshev distance", off.min(), "of", len(on_dev))
    assert (off == 0).any()
    full = _fitter(im, seeds)
    full.firstfit()
    full.repeatfit()
    with full.residual_stack("add") as st:
        none_left = get_seeds(st, th_seed=600)
    full.release()
    assert not len(none_left) or np.abs(none_left - seeds[k]).max(1).min() > 1   # fitted, the blob is gone from the residual


# ---- 8 -----------------------------------------------------------------------------------------------------------------
def test_lifetime_and_release():
    im, seeds, first, fo = VR.oracle_fit("edge_f32")
    f = _fitter(im, seeds)
    f.firstfit()
    f.repeatfit()
    recs = f.ims_rec                                               # still there after repeatfit()
    add = f.im_add
    assert add.tobytes() == VR.residual(im, seeds, recs, RADIUS).tobytes()
    ps = np.array(f.ps)
    f.release()
    assert f.ims_rec is recs and f.im_add is add and np.array_equal(np.array(f.ps), ps, equal_nan=True)
    for attr in ("gparms", "im_subtr"):
        with pytest.raises(AttributeError, match="released"):
            getattr(f, attr)
    with pytest.raises(AttributeError, match="released"):
        f.residual_stack("add")
    f.release()                                                    # twice is fine
    # no seeds: firstfit() leaves nothing behind (the reference's own firstfit() fails on im_subtr there)
    e = _fitter(im, np.zeros((0, 3)))
    e.firstfit()
    for attr in ("gparms", "ims_rec", "im_subtr", "im_add"):
        with pytest.raises(AttributeError):
            getattr(e, attr)
    # a new firstfit() drops what was rendered
    f2 = _fitter(im, seeds)
    f2.firstfit()
    a = f2.im_add
    f2.firstfit()
    assert "im_add" not in f2.__dict__ and f2.im_add is not a and f2.im_add.tobytes() == a.tobytes()


def _ws_stats():
    from imageanalysis3_amd import _lib as L
    s = (C.c_double * 6)()
    L.check(L.lib().ia3_workspace_stats(s))
    return [float(v) for v in s][:5]      # idle bytes, bytes in use, blocks, hipMalloc calls, hipFree calls


# {idle bytes, bytes in use, blocks, hipMalloc calls, hipFree calls} of the scratch cache after fit_fov_image on c1_u16
# (30 x 128 x 128 uint16 host array, 50 seeds) in a fresh process, as the PARENT commit leaves them — after the first call
# and unchanged after the second and the third (measured with the parent's package and library on the MI355X)
PARENT_STATS = [24801568.0, 0.0, 13.0, 13.0, 0.0]

_FOOTPRINT_CHILD = """
import sys, json, ctypes as C
sys.path[:0] = [%r, %r]
from conftest import build_case
from imageanalysis3_amd import _lib as L
from imageanalysis3_amd.spot_tools.fitting import fit_fov_image
L.check(L.lib().ia3_init(0))
im = build_case("c1_u16")
out = []
for k in range(2):
    t = fit_fov_image(im, "647", th_seed=600, max_num_seeds=None, verbose=False)
    s = (C.c_double * 6)()
    L.check(L.lib().ia3_workspace_stats(s))
    out.append([float(v) for v in s][:5] + [len(t)])
print("STATS " + json.dumps(out))
"""


def test_fit_fov_image_footprint_is_the_parents():
    """fit_fov_image on a host array keeps no view (keep_views = False, release() once the rows are taken), so what it
    asks of the scratch cache is what the parent commit asked: in a fresh child process, after the first call and again
    after the second, the five figures are PARENT_STATS.  A snapshot block, or a fitter that is not released, adds a
    block and a hipMalloc call and fails this.  (The test is about a fresh process, hence the child.)"""
    import json
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-c", _FOOTPRINT_CHILD % (os.path.dirname(here), here)], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("STATS ")][-1]
    stats = json.loads(line[6:])
    print("workspace after fit_fov_image, fresh process:", stats, "parent:", PARENT_STATS)
    assert [s[5] for s in stats] == [50, 50]
    assert stats[0][:5] == PARENT_STATS and stats[1][:5] == PARENT_STATS


def test_views_give_their_scratch_back():
    """A fitter that rendered every view and was released leaves no byte of the scratch cache in use, and a caller's
    DeviceStack that was freed under the fitter is refused, not read."""
    from imageanalysis3_amd import _lib as L
    im, seeds, first, fo = VR.oracle_fit("c1_u16")
    before = _ws_stats()
    f = _fitter(im, seeds)
    f.firstfit()
    f.repeatfit()
    f.gparms, f.ims_rec, f.im_subtr, f.im_add
    f.residual_stack("add").free()
    f.release()
    after = _ws_stats()
    print("workspace around a fitter with views:", before, "->", after)
    assert after[1] == before[1]
    st = L.DeviceStack.upload(im)
    f = _fitter(st, seeds)
    f.firstfit()
    recs = f.ims_rec
    st.free()
    assert f.ims_rec is recs
    with pytest.raises(AttributeError, match="freed"):
        f.im_add
    with pytest.raises(AttributeError, match="freed"):
        f.residual_stack("subtr")
    f.release()


# ---- 9 -----------------------------------------------------------------------------------------------------------------
def test_legacy_class_identities():
    """External/Fitting_v3.iter_fit_seed_points (model_variant 1: its to_center, per-axis start widths) inherits the views:
    test 2's identities on the arguments tests/test_gpu_parity.py fits it with."""
    from imageanalysis3_amd.External import Fitting_v3
    from imageanalysis3_amd import visual_tools as vt
    im, m = build_legacy()
    g = load_golden("legacy.npz")
    sa = tuple(m["seeding"]["default"][:-1]) + (False,)
    fa = tuple(m["fitting_args"])
    s = vt.get_seed_in_distance(im, g["coords"][0], *sa)
    assert len(s) >= 2 and fa[0] == RADIUS
    seeds = np.asarray(s, dtype=np.float64)[:, :3]
    a = _identities(im, seeds, lambda: Fitting_v3.iter_fit_seed_points(im, s.T, *fa))
    b = _identities(im, seeds, lambda: Fitting_v3.iter_fit_seed_points(im, s.T, *fa))
    assert a == b


def test_multi_field_fitter_is_refused():
    from imageanalysis3_amd import _lib as L
    im, seeds, first, fo = VR.oracle_fit("edge_f32")
    lib = L.lib()
    c = np.ascontiguousarray(seeds, dtype=np.float64)
    with L.DeviceStack.upload(im) as s1, L.DeviceStack.upload(im) as s2:
        ims = (C.c_void_p * 2)(s1._h.value, s2._h.value)
        cen = (C.c_void_p * 2)(c.ctypes.data, c.ctypes.data)
        ns = (C.c_int * 2)(len(c), len(c))
        p = L.make_fit_params(RADIUS)
        h = C.c_void_p()
        L.check(lib.ia3_fit_create_fovs(ims, cen, ns, 2, C.byref(p), C.byref(h)))
        try:
            L.check(lib.ia3_fit_first(h))
            n = 2 * len(c)
            ps = np.empty((n, 11), dtype=np.float32)
            L.check(lib.ia3_fit_results(h, L.ptr(ps), None, None))
            assert np.array_equal(ps[:len(c)], ps[len(c):], equal_nan=True)      # two fields, the same image
            np.testing.assert_allclose(ps[:len(c), :8], first["ps"][:, :8], rtol=1e-4)
            out = np.empty(im.shape, dtype=np.float64)
            cnt = np.empty(n, dtype=np.int32)
            with pytest.raises(NotImplementedError, match="one field of view"):
                L.check(lib.ia3_fit_snapshot(h))
            with pytest.raises(NotImplementedError):
                L.check(lib.ia3_fit_view_residual(h, 1, L.dptr(out)))
            with pytest.raises(NotImplementedError):
                L.check(lib.ia3_fit_view_voxels(h, L.ptr(cnt), L.ptr(cnt), L.dptr(out)))
            with pytest.raises(NotImplementedError):
                L.check(lib.ia3_fit_view_recs(h, 1, L.ptr(cnt), L.ptr(cnt.view(np.uint8)), L.dptr(out), None))
            st = C.c_void_p()
            with pytest.raises(NotImplementedError):
                L.check(lib.ia3_fit_view_residual_dev(h, 1, C.byref(st)))
        finally:
            lib.ia3_fit_destroy(h)
