"""CPU: the chromosome image without a device.  tests/harness/chromim_ref.py (the NumPy / SciPy statement of
classes/field_of_view.py:1853-1901) reproduces the reference's own outputs (tests/golden/chromim.npz, written by
scripts/make_chrom_image_golden.py); the rules the kernels rely on are pinned against the installed NumPy and SciPy; the flat
forms have the documented signatures and refuse bad arguments before they touch the device; the candidate cases of the GPU
tests are not empty."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
from scipy import ndimage

from conftest import load_golden
from harness import chromim_cases as K
from harness import chromim_ref as R
from harness import chromseg_ref as S

E = inspect.Parameter.empty


@pytest.fixture(scope="module")
def gold():
    return load_golden("chromim.npz")


def test_statement_reproduces_the_reference_outputs(gold):
    assert str(gold["source"]) == "reference"
    for key, (name, count, _, _) in K.FILES.items():
        shape = K.SHAPES[name]
        ims, fl, dr = K.case(name, count)
        got = R.chrom_im(ims, fl, dr, shape)
        want = gold[key + "_fast"]
        assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), key
        assert R.shifted_sum(ims, fl, dr, shape).tobytes() == want.tobytes(), key      # order-free
        cvals = {id(im): c for im, c in zip(ims, gold[key + "_cvals"])}
        slow = R.chrom_im(ims, fl, dr, shape, fast=False, background=lambda im: cvals[id(im)])
        assert slow.tobytes() == gold[key + "_slow"].tobytes(), key
        assert (slow != want).any()


def test_rounding_is_half_to_even_on_the_stored_dtype():
    d = np.array([0.5, 1.5, 2.5, -0.5, -1.5], dtype=np.float32)
    assert np.round(d).astype(int).tolist() == [0, 2, 2, 0, -2]
    assert np.round([d[:3], d[2:]]).dtype == np.float32            # a list of the file's rows stays float32


def test_every_partial_sum_is_exact():
    ims, fl, dr = K.case("even", 10)
    a = R.chrom_im(ims, fl, dr, K.SHAPES["even"])
    assert np.array_equal(a * 2, np.round(a * 2)) and a.max() < 2.0 ** 52
    Y = K.SHAPES["even"][2]
    with pytest.raises(ValueError, match="broadcast"):
        R.chrom_im(ims[:1], [1], np.array([[0, 0, Y + 1]], np.float32), K.SHAPES["even"])
    # at |d| = N exactly both crops are empty and NumPy adds the median everywhere; the flat form refuses |d| >= N
    assert (R.chrom_im(ims[:1], [1], np.array([[0, 0, -Y]], np.float32), K.SHAPES["even"]) == np.median(ims[0])).all()
    for name, shape in K.SHAPES.items():
        med = {k: float(np.median(v)) for k, v in K.median_images(shape).items()}
        assert med["constant"] == 731.0 and med["equal"] == 400.0 and med.get("half", 400.5) == 400.5
        assert ("half" in med) == (int(np.prod(shape)) % 2 == 0)


@pytest.mark.parametrize("name", sorted(K.SHAPES))
def test_shift_is_map_coordinates_at_grid_plus_drift(name):
    """What lets ``fast=False`` run on the order-1 constant warp: identical bytes, cval rounded the same way."""
    shape = K.SHAPES[name]
    ims, _, dr = K.slow_case(name)
    grid = np.indices(shape).astype(np.float64)
    for im, d, c in zip(ims, dr, (400.0, 400.5, 401.49, 0.0, 412.5)):
        d = np.asarray(d, dtype=np.float64)
        a = ndimage.shift(im, -d, order=1, mode='constant', cval=c)
        b = ndimage.map_coordinates(im, grid + d[:, None, None, None], order=1, mode='constant', cval=c)
        assert a.dtype == np.uint16 and a.tobytes() == b.tobytes()
    assert (ndimage.shift(ims[4], -dr[4].astype(np.float64), order=1, mode='constant', cval=412.5) == 413).all()   # all cval


SIGNATURES = {
    "generate_chrom_im": [("ims", E), ("flags", E), ("drifts", E), ("single_im_size", None), ("fast", True),
                          ("chrom_im", None), ("return_device", False)],
    "generate_chrom_im_from_data": [("save_filename", E), ("data_type", E), ("num_loaded_image", 10), ("fast", True),
                                    ("image_dtype", np.uint16), ("return_device", False), ("verbose", True)],
}


def test_names_and_signatures():
    from imageanalysis3_amd.classes import field_of_view as F
    for name, want in SIGNATURES.items():
        got = [(p.name, p.default) for p in inspect.signature(getattr(F, name)).parameters.values()]
        assert got == want, (name, got)
    with pytest.raises(ImportError):
        from imageanalysis3_amd.classes.field_of_view import Field_of_View  # noqa: F401
    from imageanalysis3_amd import _lib
    for name in ("empty", "upload", "download", "add", "free", "__enter__", "__exit__"):
        assert callable(getattr(_lib.ChromImage, name))
    assert callable(_lib.stack_median) and _lib.CHROM_ADD_BATCH == 16


def test_ctypes_mirrors_match_the_header():
    """Every new entry is declared in include/ia3.h (test_abi_cpu.py checks the prototypes of all entries)."""
    import re
    from imageanalysis3_amd import _lib
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "ia3.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _lib.lib()
    for name in ("ia3_chrom_image_create", "ia3_chrom_image_free", "ia3_chrom_image_upload", "ia3_chrom_image_download",
                 "ia3_chrom_image_add_dev", "ia3_stack_median_dev", "ia3_find_candidate_chromosomes_f64_dev"):
        assert re.search(r"\b%s\s*\(" % name, src) and name in _lib.EXPORTS and hasattr(lib, name)
    assert lib.ia3_chrom_image_free.restype is None
    # the f64 entry takes what the uint16 / float32 entry takes, the image handle aside
    a = re.search(r"ia3_find_candidate_chromosomes_dev\s*\(([^)]*)\)", src).group(1).split(",")[1:]
    b = re.search(r"ia3_find_candidate_chromosomes_f64_dev\s*\(([^)]*)\)", src).group(1).split(",")[1:]
    assert [" ".join(x.split()) for x in a] == [" ".join(x.split()) for x in b]
    assert C.sizeof(_lib.ChromParams) == 24


def test_argument_errors_before_the_device(monkeypatch, tmp_path):
    from imageanalysis3_amd import _lib
    from imageanalysis3_amd.classes import field_of_view as F
    from imageanalysis3_amd.segmentation_tools import chromosome as CH

    def no_device(*a, **k):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(_lib.DeviceStack, "upload", classmethod(no_device))
    monkeypatch.setattr(_lib.ChromImage, "empty", classmethod(no_device))
    monkeypatch.setattr(_lib, "lib", no_device)
    shape = K.SHAPES["odd"]
    ims, fl, dr = K.case("odd", 10)
    for axis in range(3):
        for sign in (1, -1):
            d = dr.copy()
            d[3] = 0
            d[3, axis] = sign * (shape[axis] - 0.4)          # rounds to the axis length
            with pytest.raises(ValueError, match="broadcast"):
                F.generate_chrom_im(ims, fl, d)
    with pytest.raises(IndexError):
        F.generate_chrom_im(ims[:2] + [ims[2][:, :, :-1]], fl[:3], dr[:3])
    with pytest.raises(IndexError):
        F.generate_chrom_im(ims[:2], fl[:2], dr[:2], single_im_size=(5, 19, 36))
    with pytest.raises(NotImplementedError, match="uint16"):
        F.generate_chrom_im([ims[0], ims[1].astype(np.float32)], fl[:2], dr[:2])
    with pytest.raises(NotImplementedError, match="uint16"):
        F.generate_chrom_im([ims[0].astype(np.float64)], fl[:1], dr[:1])
    for bad in ([[0]], "im.npy", None):
        with pytest.raises(TypeError):
            F.generate_chrom_im([bad], fl[:1], dr[:1])
        with pytest.raises(TypeError):
            F.generate_chrom_im([ims[0], bad], fl[:2], dr[:2])
    with pytest.raises(TypeError):
        F.generate_chrom_im(ims[:1], fl[:1], dr[:1], chrom_im=np.zeros(shape))
    with pytest.raises(ValueError):
        F.generate_chrom_im(ims[:2], fl[:1], dr[:2])
    with pytest.raises(ValueError):
        F.generate_chrom_im([], [], [])
    # a flag-2 image is added as it is: its drift is not looked at
    d = dr[:1].copy()
    d[0] = 1000
    with pytest.raises(AssertionError, match="device"):
        F.generate_chrom_im(ims[:1], [2], d)
    with pytest.raises(ValueError, match="Wrong input data_type: chrom"):
        F.generate_chrom_im_from_data(str(tmp_path / "none.hdf5"), "chrom")
    with pytest.raises(NotImplementedError):
        F.generate_chrom_im_from_data(str(tmp_path / "none.hdf5"), "unique", image_dtype=np.float32)
    with pytest.raises(IOError):
        F.generate_chrom_im_from_data(str(tmp_path / "none.hdf5"), "unique")
    for bad in (np.zeros(shape, np.float32), [[0.0]], "x"):
        with pytest.raises(TypeError):
            _lib.ChromImage.upload(bad)
    with pytest.raises(IndexError):
        _lib.ChromImage.upload(np.zeros((4, 4)))
    # what find_candidate_chromosomes did with a float64 ndarray stays
    f64 = ims[0].astype(np.float64) / 7
    with pytest.raises(NotImplementedError, match="exact in float32"):
        CH.find_candidate_chromosomes(f64, _verbose=False)


def test_candidate_cases_are_not_empty():
    """Every candidate case of tests/test_gpu_chrom_image.py finds at least three objects and loses at least one label to
    the size filter, by the statement alone; the "seventh" images are not exact in float32."""
    images = {}
    for key, name, kind, fs, per in K.candidate_cases():
        if name not in images:
            ims, fl, dr = K.round_copies(name)
            images[name] = R.chrom_im(ims, fl, dr, ims[0].shape)
        a = images[name] if kind == "sum" else images[name] / 7
        assert a.dtype == np.float64
        exact32 = np.array_equal(a.astype(np.float32).astype(np.float64), a)
        assert exact32 == (kind == "sum"), key
        st = S.chain(a, fs, per, 1, K.CAND_MIN_SIZE)
        assert len(st["ids"]) >= 3 and len(st["ids"]) < st["n"], (key, len(st["ids"]), st["n"])
    assert {k[2] for k in K.candidate_cases()} == {"sum", "seventh"} and {k[1] for k in K.candidate_cases()} == {"small", "large"}
