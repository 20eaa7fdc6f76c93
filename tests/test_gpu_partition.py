"""GPU: the label kernels (labels.hip) and what is built on them — bounding boxes and counts of a label stack, the vote /
contains / max / gather over the clamped cubes around spots, the per-cell spot caller ``fit_spots_by_segmentation`` and
``fit_fov_image`` with a resident seed mask.  Everything here is integer work or the same operators on the same crops:
every comparison is exact (the one exception is the reference's own fit rows of tests/golden/seg.npz, held to the bar of
tests/test_gpu_parity.py).  The reference's outputs are tests/golden/partition.npz; inputs it does not cover compare
with the NumPy statement tests/harness/partition_ref.py, which tests/test_partition_cpu.py holds to the same file."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden
from harness import partition_cases as PC
from harness import partition_ref as PR

pytestmark = pytest.mark.gpu

RADII = (0, 1, 3, 4, 10)
RTOL = 1e-4


@pytest.fixture(scope="module")
def gold():
    return load_golden("partition.npz")


@pytest.fixture(scope="module")
def labels():
    return PC.label_cases()


@pytest.fixture(scope="module")
def ref_boxes(labels):
    """np.bincount + per-label np.nonzero bounds of every case, computed once."""
    return {name: PR.boxes(lab, 65535) for name, lab in labels.items()}


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# copies of the helpers of tests/test_gpu_parity.py
def match_rows(a, b, tol=0.05):
    from scipy.spatial import cKDTree
    assert len(a) == len(b), (len(a), len(b))
    if len(a) == 0:
        return np.zeros(0, int), np.zeros(0, int)
    d, j = cKDTree(b[:, 1:4]).query(a[:, 1:4])
    assert (d < tol).all(), d.max()
    assert len(np.unique(j)) == len(j)
    return np.arange(len(a)), j


def assert_rows_close(a, b, rtol=RTOL):
    ia, ib = match_rows(a, b)
    a, b = a[ia].astype(np.float64), b[ib].astype(np.float64)
    rel = np.abs(a[:, :8] - b[:, :8]) / np.abs(b[:, :8])
    assert rel.max() <= rtol, ("max rel err %g at %s" % (rel.max(), np.unravel_index(rel.argmax(), rel.shape)))
    assert np.abs(a[:, 8:10] - b[:, 8:10]).max() <= 2e-3
    assert (np.abs(a[:, 10] - b[:, 10]) / np.abs(b[:, 10])).max() <= 1e-3


# ---------------------------------------------------------------------------------------------------------------------
# boxes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["seg", "small", "distinct", "one"])
def test_label_boxes_exact_and_repeatable(name, labels, ref_boxes, gold):
    """One pass gives np.bincount and the per-label np.nonzero bounds exactly, the same bits on two runs: runs that change
    inside a wavefront and across two, rows that are no multiple of 64, a workgroup table that overflows (every voxel a
    label of its own), one voxel."""
    from imageanalysis3_amd import _lib as L
    from imageanalysis3_amd.segmentation_tools.cell import segmentation_label_boxes, segmentation_mask_2_bounding_box
    lab = labels[name]
    with L.DeviceStack.upload(lab.astype(np.uint16)) as st:
        t1 = L.label_boxes(st, 65535)
        t2 = L.label_boxes(st, 65535)
        assert _same(t1, t2)
        assert t1.dtype == np.int32 and np.array_equal(t1, ref_boxes[name]), np.nonzero((t1 != ref_boxes[name]).any(axis=1))[0][:10]
        top = int(lab.max()) - 1   # labels above max_label are passed over, the others are unchanged
        if top >= 1:
            assert np.array_equal(L.label_boxes(st, top), ref_boxes[name][:top + 1])
        ids, boxes, counts = segmentation_label_boxes(st)
        assert _same(ids, gold[name + "_ids"]) and _same(boxes, gold[name + "_boxes"])
        assert np.array_equal(counts, np.bincount(lab.ravel())[ids])
        assert np.array_equal(segmentation_mask_2_bounding_box(st, None, 2).array, gold[name + "_union_box"])
    ids2, boxes2, counts2 = segmentation_label_boxes(lab, extend_pixel=0)   # the host array (int32) through the same pass
    assert np.array_equal(boxes2, ref_boxes[name][ids2, 1:].reshape(-1, 3, 2)) and np.array_equal(counts2, counts)
    for l, b in list(zip(ids, gold[name + "_boxes"]))[:3]:
        crop = segmentation_mask_2_bounding_box(lab, int(l))
        assert np.array_equal(crop.array, b) and tuple(crop.image_sizes) == lab.shape
        assert np.array_equal(segmentation_mask_2_bounding_box(lab == l, 3).array, b)   # the call of preprocess.py:1117


def test_label_boxes_unaligned_stack_and_argument_errors(ref_boxes):
    """A borrowed stack that does not start on a 16-byte boundary takes the plain loads: same table.  Bad arguments."""
    from imageanalysis3_amd import _lib as L
    lab = PC.small_labels().astype(np.uint16)
    flat = np.zeros((1, 1, lab.size + 3), np.uint16)
    flat[0, 0, 3:] = lab.ravel()
    with L.DeviceStack.upload(flat) as st:
        d = C.c_void_p()
        L.check(L.lib().ia3_stack_info(st._h, None, None, None, None, C.byref(d)))
        h = C.c_void_p()
        L.check(L.lib().ia3_stack_wrap(C.c_void_p(d.value + 6), L.IA3_U16, lab.shape[0], lab.shape[1], lab.shape[2], C.byref(h)))
        view = L.DeviceStack(h, lab.shape, np.uint16)
        try:
            assert np.array_equal(L.label_boxes(view, 65535), ref_boxes["small"])
        finally:
            view.free()
        for bad in (0, 65536, -1):
            with pytest.raises(ValueError):
                L.label_boxes(st, bad)
    with L.DeviceStack.upload(lab.astype(np.float32)) as f32:
        with pytest.raises(ValueError):
            L.label_boxes(f32, 10)
        with pytest.raises(ValueError):
            L.cube_labels(f32, np.zeros((1, 3)), 1)
        for r in (-1, 11):
            with pytest.raises(ValueError):
                L.cube_max(f32, np.zeros((1, 3)), r)
            with pytest.raises(ValueError):
                L.cube_gather(f32, np.zeros((1, 3)), r)


# ---------------------------------------------------------------------------------------------------------------------
# cubes around spots
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["seg", "small", "distinct", "one"])
def test_vote_contains_gather_exact(name, labels, gold):
    """Centres on .5 boundaries, at the eight corners, outside the image (the cube collapses onto a face), in a two-label
    tie, in an all-background cube; on the all-distinct stack a counter per label is needed.  Against the reference's
    outputs where the fixture has them and against the NumPy statement at every radius."""
    from imageanalysis3_amd import _lib as L
    from imageanalysis3_amd.classes.partition_spots import find_coordinate_intensities, Spots_Partition as SP
    from imageanalysis3_amd.classes.preprocess import Spots3D
    lab = labels[name]
    coords = gold[name + "_coords"]
    ids = gold[name + "_ids"]
    with L.DeviceStack.upload(lab.astype(np.uint16)) as st:
        for r in RADII:
            want = PR.vote(lab, coords, r)
            key = "%s_labels_r%d" % (name, r)
            if key in gold:
                assert np.array_equal(want, gold[key])
            got = L.cube_labels(st, coords, r)
            assert _same(got, want), (r, np.nonzero(got != want)[0][:10])
            assert _same(L.cube_labels(st, coords, r), got)
            # contains: the label each cube votes for (or one that is nowhere), and labels dealt round the spots
            for target in (np.where(want > 0, want, 65534), ids[np.arange(len(coords)) % len(ids)]):
                assert _same(L.cube_labels(st, coords, r, target=target), PR.contains(lab, coords, r, target)), r
            wantm = PR.gather(lab, coords, r)
            key = "%s_fci_r%d" % (name, r)
            if key in gold:
                assert np.array_equal(wantm, gold[key])
            gotm = L.cube_gather(st, coords, r)
            assert gotm.dtype == np.uint16 and np.array_equal(gotm, wantm), r
            assert np.array_equal(L.cube_max(st, coords, r), wantm.max(axis=1))
        # the public names: resident stack and host array (int32: carried as uint16, handed back as int32)
        spots = Spots3D(PC.spot_table(coords, np.float32))
        v = SP.spots_to_labels(st, spots, search_radius=3, verbose=False)
        assert _same(v, gold[name + "_labels_r3"])
    table = PC.spot_table(coords)
    assert _same(SP.spots_to_labels(lab, table, verbose=False), gold[name + "_labels_r10"])
    assert _same(SP.spots_to_labels(lab, table, search_radius=4, verbose=False), gold[name + "_labels_r4"])
    assert _same(find_coordinate_intensities(lab, table, search_radius=1), gold[name + "_fci_r1"])
    neg = lab.astype(np.int64)
    neg[lab == ids[0]] = -3   # negative labels are background for the vote
    assert _same(SP.spots_to_labels(neg, table, search_radius=3, verbose=False), PR.vote(np.maximum(neg, 0), coords, 3))


def test_tie_and_background_spots(gold):
    from imageanalysis3_amd.classes.partition_spots import Spots_Partition as SP
    lab = PC.small_labels()
    coords = gold["small_coords"]
    k, b = PC.special_index("small", "tie", lab.shape), PC.special_index("small", "background", lab.shape)
    for r in (1, 3, 4):
        cube = PR.gather(lab, coords[k:k + 1], r)[0]
        assert (cube == 9).sum() == (cube == 5).sum() > 0   # label 9 comes first in the cube, label 5 is the smaller
        v = SP.spots_to_labels(lab, PC.spot_table(coords[[k, b]]), search_radius=r, verbose=False)
        assert v.tolist() == [5, -1]


@pytest.mark.parametrize("tag", ["u16", "f32", "nan"])
def test_cube_max_exact(tag, gold):
    """spots_to_DAPI on uint16 and float32 stacks; a NaN in the cube gives NaN, as np.max does."""
    from imageanalysis3_amd import _lib as L
    from imageanalysis3_amd.classes.partition_spots import find_coordinate_intensities, Spots_Partition as SP
    im = {"u16": PC.dapi_u16, "f32": PC.dapi_f32, "nan": lambda: PC.dapi_f32(nan=True)}[tag]()
    coords = gold["dapi_coords"]
    table = PC.spot_table(coords)
    with L.DeviceStack.upload(im) as st:
        for r in (0, 1, 3, 4, 5, 10):
            want = PR.cube_max(im, coords, r)
            key = "dapi_%s_r%d" % (tag, r)
            if key in gold:
                assert np.array_equal(want, gold[key], equal_nan=True)
            got = SP.spots_to_DAPI(st, table, search_radius=r, verbose=False)
            assert got.dtype == im.dtype and np.array_equal(got, want, equal_nan=True), r
            if tag == "nan":
                assert np.array_equal(np.isnan(got), np.isnan(PR.gather(im, coords, r)).any(axis=1))
        assert np.isnan(SP.spots_to_DAPI(st, table, search_radius=10, verbose=False)).any() == (tag == "nan")
        m = find_coordinate_intensities(st, table, search_radius=3)
        assert m.dtype == im.dtype and np.array_equal(m, PR.gather(im, coords, 3), equal_nan=True)
    got = SP.spots_to_DAPI(im, table, verbose=False)   # the host array, default radius
    assert got.dtype == im.dtype and np.array_equal(got, gold["dapi_%s_r5" % tag], equal_nan=True)
    if tag == "u16":   # an int64 copy travels as uint16 and comes back as int64
        got = SP.spots_to_DAPI(im.astype(np.int64), table, verbose=False)
        assert got.dtype == np.int64 and np.array_equal(got, gold["dapi_u16_r5"])


def test_no_spots_launch_nothing():
    from imageanalysis3_amd import _lib as L
    with L.DeviceStack.upload(PC.small_labels().astype(np.uint16)) as st:
        none = np.zeros((0, 3))
        assert L.cube_labels(st, none, 3).shape == (0,)
        assert L.cube_labels(st, none, 3, target=np.zeros(0, np.int32)).shape == (0,)
        assert L.cube_max(st, none, 10).shape == (0,)
        assert L.cube_gather(st, none, 2).shape == (0, 125)
        rc = L.lib().ia3_cube_gather_dev(st._h, None, 0, 2, None)
        assert rc == L.IA3_OK


# ---------------------------------------------------------------------------------------------------------------------
# the callers
# ---------------------------------------------------------------------------------------------------------------------
def test_fit_spots_by_segmentation_golden_and_replay(tmp_path):
    """classes/preprocess.py:1093-1153 on the chain case, the three calls of the reference's run (tests/golden/seg.npz): no
    drift, a drift with num_spots = 2, a 3-voxel label whose box holds no seed.  Ids equal the reference's, rows meet the
    bar of the parity tests; rows and ids equal the flat replay (label image on the host, one mask per cell) bit for bit;
    a resident label stack gives what the host label image gives."""
    from conftest import seg_labels, build_chain_case, write_dax
    from harness import replay as R
    from imageanalysis3_amd import _lib as L
    from imageanalysis3_amd.classes.preprocess import fit_spots_by_segmentation
    g = load_golden("seg.npz")
    case = build_chain_case()
    size = [case["Z"], case["X"], case["Y"]]
    lab = seg_labels(size)
    drift = np.array(case["drift"])
    path = str(tmp_path / "movie.dax")
    write_dax(path, case["raw"])
    st = R.load_channels(path, case["chs"], case["chs"], size, n_buffer=case["nb"])
    try:
        R.hot_pixels_in_image_dtype(st, case["chs"])
        calls = {"647": (lab, np.zeros(3), dict(th_seed=300, segment_search_radius=3)),
                 "750": (lab, drift, dict(th_seed=300, num_spots=2)),
                 "561": ((lab == 4) * 4, drift, dict(th_seed=300))}
        for ch, (seg, dft, kw) in calls.items():
            rkw = dict(th_seed=kw["th_seed"], num_spots=kw.get("num_spots"), search_radius=kw.get("segment_search_radius", 3))
            want_s, want_i = R.fit_in_labels(st[ch], ch, seg, dft, **rkw)
            got_s, got_i = fit_spots_by_segmentation(st[ch], ch, seg, drift=dft, **kw)
            assert _same(got_s, want_s) and _same(got_i, want_i), ch
            with L.DeviceStack.upload(seg.astype(np.uint16)) as dev_seg:
                res_s, res_i = fit_spots_by_segmentation(st[ch], ch, dev_seg, drift=dft, **kw)
            assert _same(res_s, got_s) and _same(res_i, got_i), ch
            host_s, host_i = fit_spots_by_segmentation(st[ch].download(), ch, seg, drift=dft, **kw)   # the image from the host
            assert _same(host_s, got_s) and _same(host_i, got_i), ch
            if ch == "561":
                assert len(got_s) == 0 and len(got_i) == 0 and g["spots_561"].shape == (0,)
            else:
                assert got_i.dtype == np.int32 and np.array_equal(got_i, g["ids_" + ch])
                assert got_s.dtype == np.float32 and got_s.shape[1] == 11
                assert_rows_close(np.asarray(got_s), g["spots_" + ch])
        s0, i0 = fit_spots_by_segmentation(st["647"], "647", lab, th_seed=300)   # drift=None is no drift
        w0, wi0 = R.fit_in_labels(st["647"], "647", lab, np.zeros(3), th_seed=300)
        assert _same(s0, w0) and _same(i0, wi0)
    finally:
        R.free_all(st)


@pytest.mark.parametrize("name", ["c1_f32", "c1_u16"])
def test_fit_fov_image_resident_seed_mask(name):
    """spot_tools/fitting.py:210-218 with the mask resident: the radius-0 lookup selects the seeds the host indexing
    selects, so the tables are equal bit for bit (mask of the seedopts fixture, float32 and as a uint16 stack)."""
    from conftest import build_case, seed_mask_for
    from imageanalysis3_amd import _lib as L
    from imageanalysis3_amd.spot_tools.fitting import fit_fov_image
    g = load_golden("seedopts.npz")
    im = build_case(name)
    mask = seed_mask_for(im.shape)
    want = fit_fov_image(im, "647", th_seed=600, max_num_seeds=None, seed_mask=mask, verbose=False)
    assert want.shape == g[name + "_mask_table"].shape and len(want) > 0
    with L.DeviceStack.upload(mask) as dm, L.DeviceStack.upload((mask > 0).astype(np.uint16)) as dm16, \
            L.DeviceStack.upload(im) as dim:
        assert _same(fit_fov_image(im, "647", th_seed=600, max_num_seeds=None, seed_mask=dm, verbose=False), want)
        assert _same(fit_fov_image(dim, "647", th_seed=600, max_num_seeds=None, seed_mask=dm16, verbose=False), want)
        seeds = load_golden("fit_%s.npz" % name)["seeds_h"]
        given = fit_fov_image(im, "647", seeds=seeds, seed_mask=mask > 0, verbose=False)
        assert _same(fit_fov_image(im, "647", seeds=seeds, seed_mask=dm16, verbose=False), given)
    with L.DeviceStack.upload(np.zeros((2, 3, 4), np.uint16)) as wrong:
        with pytest.raises(IndexError):
            fit_fov_image(im, "647", th_seed=600, max_num_seeds=None, seed_mask=wrong, verbose=False)


def test_fit_spots_by_segmentation_compiles_nothing(tmp_path, capfd, monkeypatch):
    """Crops of depths without a built-in column kernel (19 and 17 planes) take the sliding-window pass on this route: no
    kernel is compiled at run time (the cache folder stays empty, the library announces nothing) and the tables are the
    replay's with the column kernels switched off (IA3_TUNE_GAUSS_FOLD = 0: the same pass for every depth), bit for bit."""
    from harness import replay as R
    from imageanalysis3_amd import _lib as L, synth
    from imageanalysis3_amd.classes.preprocess import fit_spots_by_segmentation
    monkeypatch.setenv("IA3_RTC_CACHE", str(tmp_path))
    shape = (21, 64, 64)
    im = synth.make_fov(shape, 8, 5, dtype=np.uint16, margin=(3, 6, 6))[0]
    lab = np.zeros(shape, np.int32)
    lab[2:19, 2:30, 2:62] = 1    # box with its margin: planes 1..19, depth 19
    lab[3:18, 34:62, 2:62] = 2   # depth 17
    with L.DeviceStack.upload(im) as st:
        got_s, got_i = fit_spots_by_segmentation(st, "647", lab, th_seed=300)
        L.check(L.lib().ia3_set_tuning(L.IA3_TUNE_GAUSS_FOLD, 0))
        try:
            want_s, want_i = R.fit_in_labels(st, "647", lab, np.zeros(3), th_seed=300)
        finally:
            L.check(L.lib().ia3_set_tuning(L.IA3_TUNE_GAUSS_FOLD, 1))
    assert len(got_s) > 0 and set(got_i.tolist()) == {1, 2}
    assert _same(got_s, want_s) and _same(got_i, want_i)
    assert list(tmp_path.iterdir()) == []
    assert "compiling" not in capfd.readouterr().err
