"""CPU: the label lookups without a device — the NumPy statement tests/harness/partition_ref.py against the reference's
own outputs (tests/golden/partition.npz, written by scripts/make_partition_golden.py) exactly, the index arithmetic the
kernels compile (csrc/ia3_labels.h, built for the host by tests/native/labels_cpu.cpp) against that statement, and the
package's argument handling: names, signatures, dtype rules, errors and empty tables."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

from conftest import load_golden
from harness import partition_cases as PC
from harness import partition_ref as PR

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "native", "liblabelscpu.so")
E = inspect.Parameter.empty


@pytest.fixture(scope="module")
def native():
    src = os.path.join(HERE, "native", "labels_cpu.cpp")
    dep = os.path.join(HERE, "..", "imageanalysis3_amd", "csrc", "ia3_labels.h")
    if not os.path.isfile(SO) or os.path.getmtime(SO) < max(os.path.getmtime(src), os.path.getmtime(dep)):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", SO, src])
    return C.CDLL(SO)


@pytest.fixture(scope="module")
def gold():
    return load_golden("partition.npz")


@pytest.fixture(scope="module")
def labels():
    return PC.label_cases()


def test_statement_equals_reference_lookups(gold, labels):
    n = 0
    for name, lab in labels.items():
        coords = gold[name + "_coords"]
        assert np.array_equal(coords, PC.spot_coords(name, lab.shape))
        for r in PC.FCI_RADII:
            key = "%s_fci_r%d" % (name, r)
            if key in gold:
                got = PR.gather(lab, coords, r)
                assert got.dtype == gold[key].dtype and np.array_equal(got, gold[key]), key
                n += 1
        for r in PC.VOTE_RADII:
            key = "%s_labels_r%d" % (name, r)
            got = PR.vote(lab, coords, r)
            assert got.dtype == np.int32 and np.array_equal(got, gold[key]), key
            # contains: a cube holds the label it votes for; one without a positive label holds no label 1; none holds 65534
            v = gold[key]
            assert np.array_equal(PR.contains(lab, coords, r, np.where(v > 0, v, 1)), np.where(v > 0, 1, -1)), key
            assert (PR.contains(lab, coords, r, np.full(len(coords), 65534)) == -1).all()
            n += 1
    assert n == 4 * 4 + 3 * 4 - 1
    coords = gold["dapi_coords"]
    for tag, im in (("u16", PC.dapi_u16()), ("f32", PC.dapi_f32()), ("nan", PC.dapi_f32(nan=True))):
        for r in PC.DAPI_RADII:
            got = PR.cube_max(im, coords, r)
            want = gold["dapi_%s_r%d" % (tag, r)]
            assert got.dtype == want.dtype and np.array_equal(got, want, equal_nan=True), (tag, r)


def test_statement_equals_reference_boxes(gold, labels):
    for name, lab in labels.items():
        table = PR.boxes(lab, 65535)
        ids = np.nonzero(table[:, 0])[0]
        assert np.array_equal(ids, gold[name + "_ids"])
        tight = table[ids, 1:].reshape(-1, 3, 2)
        grown = np.stack([np.maximum(tight[:, :, 0] - 1, 0), np.minimum(tight[:, :, 1] + 1, np.array(lab.shape))], axis=2)
        assert np.array_equal(grown, gold[name + "_boxes"]), name
        assert np.array_equal(table[ids, 0], np.bincount(lab.ravel())[ids])


def test_special_spots_are_what_they_claim(gold):
    lab = PC.small_labels()
    k = PC.special_index("small", "tie", lab.shape)
    for r in (3, 4):
        cube = PR.gather(lab, gold["small_coords"][k:k + 1], r)[0]
        assert (cube == 9).sum() == (cube == 5).sum() > 0 and gold["small_labels_r%d" % r][k] == 5
    for name in ("seg", "small"):
        k = PC.special_index(name, "background", PC.label_cases()[name].shape)
        assert all(gold["%s_labels_r%d" % (name, r)][k] == -1 for r in PC.VOTE_RADII)
    d10 = gold["distinct_labels_r10"]
    cubes = PR.gather(PC.distinct_labels(), gold["distinct_coords"], 10)
    # every label occurs once in the stack, but a cube that hangs over a face reads the face voxels several times (and at
    # 3 planes every cube of radius 10 does): the winner is the smallest of the labels read most often, which is the
    # smallest label of the cube only where the cube lies inside the image
    for row, won in zip(cubes, d10):
        vals, counts = np.unique(row, return_counts=True)
        assert won == vals[counts == counts.max()].min()
    assert (d10 != cubes.min(axis=1)).any()


def test_native_index_arithmetic_equals_statement(native):
    native.ia3cpu_round_centre.argtypes = [C.c_double]
    for v, want in ((2.5, 2), (3.5, 4), (-0.5, 0), (-1.5, -2), (0.49999, 0), (7.500001, 8), (-3.2, -3), (1e12, 2 ** 30), (-1e300, -2 ** 30)):
        assert native.ia3cpu_round_centre(v) == want, v
    vals = np.concatenate([np.arange(-40, 41) / 4., np.random.RandomState(0).uniform(-1e4, 1e4, 500)])
    assert [native.ia3cpu_round_centre(float(v)) for v in vals] == np.round(vals).astype(np.int32).tolist()
    for r in (0, 1, 3, 4, 10):
        off = np.empty(((2 * r + 1) ** 3, 3), dtype=np.int32)
        native.ia3cpu_cube_offsets(r, off.ctypes.data_as(C.POINTER(C.c_int)))
        assert np.array_equal(off, PR.offsets(r)), r
    for name, shape in (("small", (5, 37, 67)), ("one", (1, 1, 1)), ("seg", PC.SEG_SHAPE)):
        coords = np.ascontiguousarray(PC.spot_coords(name, shape))
        for r in (0, 1, 4, 10):
            flat = np.empty((len(coords), (2 * r + 1) ** 3), dtype=np.int64)
            native.ia3cpu_cube_voxels(coords.ctypes.data_as(C.POINTER(C.c_double)), len(coords), r, shape[0], shape[1], shape[2],
                                      flat.ctypes.data_as(C.POINTER(C.c_longlong)))
            idx = PR.cube_indices(shape, coords, r)
            assert np.array_equal(flat, np.ravel_multi_index((idx[..., 0], idx[..., 1], idx[..., 2]), shape)), (name, r)


def test_names_and_signatures():
    from imageanalysis3_amd.classes import partition_spots as P
    from imageanalysis3_amd.classes import preprocess
    from imageanalysis3_amd.segmentation_tools import cell
    want = {
        P.find_coordinate_intensities: [("image", E), ("spots", E), ("search_radius", 5)],
        P.Spots_Partition.spots_to_labels: [("segmentation_masks", E), ("spots", E), ("search_radius", 10), ("verbose", True)],
        P.Spots_Partition.spots_to_DAPI: [("dapi_im", E), ("spots", E), ("search_radius", 5), ("verbose", True)],
        cell.segmentation_mask_2_bounding_box: [("mask", E), ("cell_id", None), ("extend_pixel", 1)],
        cell.segmentation_label_boxes: [("labels", E), ("extend_pixel", 1)],
        preprocess.fit_spots_by_segmentation: [("im", E), ("channel", E), ("seg_label", E), ("drift", None), ("th_seed", 500),
                                               ("num_spots", None), ("fitting_kwargs", {}), ("segment_search_radius", 3),
                                               ("verbose", False)],
    }
    for fn, sig in want.items():
        assert [(p.name, p.default) for p in inspect.signature(fn).parameters.values()] == sig, fn
    with pytest.raises(NotImplementedError, match="classes/partition_spots.py"):
        P.Spots_Partition()
    with pytest.raises(NotImplementedError):
        P.Spots_Partition([], "x.csv")


def test_dtype_rules_before_device():
    from imageanalysis3_amd.classes.partition_spots import _device_form, find_coordinate_intensities, Spots_Partition as SP
    lab = PC.small_labels()
    spots = PC.spot_table(PC.spot_coords("small", lab.shape))
    # integer and bool images travel as uint16 and come back in their own dtype
    form, back = _device_form(lab, vote=False)
    assert form.dtype == np.uint16 and back == np.int32 and np.array_equal(form, lab)
    form, back = _device_form(lab > 0, vote=False)
    assert form.dtype == np.uint16 and back == np.bool_ and np.array_equal(form, lab > 0)
    form, back = _device_form(lab.astype(np.uint16), vote=True)
    assert form.dtype == np.uint16 and back is None
    assert _device_form(np.zeros((2, 3, 4), np.float32), vote=False)[0].dtype == np.float32
    # the vote: negative labels are background
    neg = lab.astype(np.int64)
    neg[0, 0, 0] = -5
    form, _ = _device_form(neg, vote=True)
    assert form[0, 0, 0] == 0 and np.array_equal(form.ravel()[1:], lab.ravel()[1:]) and neg[0, 0, 0] == -5
    # intensities: what does not fit in uint16 is refused
    for fn in (lambda im: find_coordinate_intensities(im, spots, 1), lambda im: SP.spots_to_DAPI(im, spots, 2, verbose=False)):
        with pytest.raises(NotImplementedError):
            fn(neg)
        with pytest.raises(NotImplementedError):
            fn(lab + 70000)
        with pytest.raises(TypeError):
            fn(lab.astype(np.float64))
        with pytest.raises(IndexError):
            fn(lab[0])
    with pytest.raises(NotImplementedError):
        SP.spots_to_labels(lab + 70000, spots, verbose=False)
    with pytest.raises(NotImplementedError):
        SP.spots_to_labels(lab.astype(np.float32), spots, verbose=False)
    with pytest.raises(NotImplementedError):
        SP.spots_to_labels(lab, spots, search_radius=11, verbose=False)
    with pytest.raises(ValueError):
        find_coordinate_intensities(lab, spots, search_radius=-1)
    with pytest.raises(IndexError):
        find_coordinate_intensities(lab, np.zeros((4, 3)), 1)


def test_empty_tables_need_no_device(capsys):
    from imageanalysis3_amd.classes.partition_spots import find_coordinate_intensities, Spots_Partition as SP
    from imageanalysis3_amd.classes.preprocess import Spots3D
    lab = PC.small_labels()
    for empty in (np.zeros((0, 11)), np.array([]), Spots3D(np.zeros((0, 11)))):
        m = find_coordinate_intensities(lab, empty, search_radius=2)
        assert m.shape == (0, 125) and m.dtype == np.int32
        assert find_coordinate_intensities(PC.dapi_f32(), empty).shape == (0, 1331)
        v = SP.spots_to_labels(lab, empty, verbose=False)
        assert v.shape == (0,) and v.dtype == np.int32
        for im in (PC.dapi_u16(), PC.dapi_f32(), lab > 0):
            v = SP.spots_to_DAPI(im, empty, verbose=False)
            assert v.shape == (0,) and v.dtype == im.dtype
    capsys.readouterr()
    SP.spots_to_labels(lab, np.zeros((0, 11)))
    assert capsys.readouterr().out == "-- partition barcodes for 0 spots\n"
