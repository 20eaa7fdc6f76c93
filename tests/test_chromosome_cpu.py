"""CPU: the candidate-chromosome path without a device.  tests/harness/chromseg_ref.py (the NumPy / SciPy statement,
scikit-image included) reproduces the reference's own outputs (tests/golden/chromosome.npz, written by
scripts/make_chromosome_golden.py); the host build of csrc/ia3_ccl.h labels, erodes and dilates like SciPy; the shim has
the reference's names and refuses what is not built before it touches the device; the window, compare and centre rules
the kernels implement are pinned against the installed SciPy and NumPy."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest
from scipy import ndimage

from conftest import load_golden
from harness import chromseg_cases as CC
from harness import chromseg_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "native", "libcclcpu.so")
E = inspect.Parameter.empty


@pytest.fixture(scope="module")
def native():
    src = os.path.join(HERE, "native", "ccl_cpu.cpp")
    dep = os.path.join(HERE, "..", "imageanalysis3_amd", "csrc", "ia3_ccl.h")
    if not os.path.isfile(SO) or os.path.getmtime(SO) < max(os.path.getmtime(src), os.path.getmtime(dep)):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", SO, src])
    return C.CDLL(SO)


@pytest.fixture(scope="module")
def gold():
    return load_golden("chromosome.npz")


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- the statement against the reference's outputs ----------------------------------------------------------------------------
def test_statement_reproduces_the_reference_outputs(gold):
    stacks = {}
    filled = closed = 0
    for key, name, dt, fs, per, ms in CC.golden_cases():
        im = stacks.setdefault((name, dt), CC.generated(name, dt))
        st = R.chain(im, fs, per, 1, ms)
        th = gold[key + "_threshold"]
        assert st["threshold"] == th and np.float64(st["threshold"]).tobytes() == th.tobytes(), key
        assert [st["n"], len(st["ids"])] == gold[key + "_n"].tolist(), key
        kept = CC.unpack_labels(gold[key + "_bits"], gold[key + "_labels"], im.shape)
        assert np.array_equal(st["kept_label"], kept), key
        assert np.array_equal(st["sizes"], gold[key + "_sizes"]), key
        want = gold[key + "_coords"]
        assert st["coords"].shape == want.shape and st["coords"].tobytes() == want.tobytes(), key
        filled += int((st["filled"] != st["opened"]).any())
        closed += int((st["closed"] != st["filled"]).any())
    # no stage of the chain is tested as an identity
    assert filled >= 8 and closed >= 8, (filled, closed)
    assert np.array_equal(R.binary_center(_center_rule_mask()), gold["center_rule"])


def _center_rule_mask():
    m = np.zeros((4, 5, 6), bool)
    m[0:2, 0:3, 0:4] = True
    return m


def test_random_walker_statement_only_covers_the_no_op():
    lab = np.array([[1, -1], [2, -1]])
    with pytest.warns(UserWarning, match="Returning provided labels"):
        assert R.random_walker(None, lab, beta=10, mode='cg_mg') is lab
    with pytest.raises(NotImplementedError):
        R.random_walker(None, np.array([[1, 0]]))


# ---- csrc/ia3_ccl.h on the host ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", CC.MASK_SHAPES)
def test_host_labelling_equals_ndimage_label(native, shape):
    for name, m in CC.masks(shape).items():
        u8 = np.ascontiguousarray(m, np.uint8)
        lab = np.empty(shape, np.int32)
        n = native.ia3cpu_label(_p(u8), *shape, _p(lab))
        ref, rn = ndimage.label(m)
        assert n == rn and np.array_equal(lab, ref), name
    m = CC.masks(shape)
    assert ndimage.label(m["edge_corner"])[1] == 4 and ndimage.label(m["serpentine"])[1] == 1
    assert ndimage.label(m["comb"])[1] == 1 and ndimage.label(m["checker"])[1] == m["checker"].sum()


def test_host_bit_rows_equal_ndimage_morphology(native):
    shape = CC.MASK_SHAPES[0]
    for name, m in CC.masks(shape).items():
        u8 = np.ascontiguousarray(m, np.uint8)
        for r in (0, 1, 2):
            for dilate in (0, 1):
                for border in (0, 1):
                    out = np.empty(shape, np.uint8)
                    native.ia3cpu_morph(_p(u8), *shape, r, dilate, border, _p(out))
                    f = ndimage.binary_dilation if dilate else ndimage.binary_erosion
                    assert np.array_equal(out.astype(bool), f(m, R.ball(r), border_value=border)), (name, r, dilate, border)


def test_ball_is_the_statement_and_ball_1_is_scipys_cross(native):
    from imageanalysis3_amd.segmentation_tools import morphology as M
    for r in (0, 1, 2):
        out = np.empty((2 * r + 1,) * 3, np.uint8)
        native.ia3cpu_ball(r, _p(out))
        assert np.array_equal(out, R.ball(r)) and np.array_equal(M.ball(r), R.ball(r)) and M.ball(r).dtype == np.uint8
    assert np.array_equal(R.ball(1).astype(bool), ndimage.generate_binary_structure(3, 1))
    assert R.ball(2).sum() == 33 and R.ball(0).shape == (1, 1, 1)


def test_host_label_sums_give_the_reference_centres(native):
    shape = CC.MASK_SHAPES[0]
    for name in ("blobs", "faces", "edge_corner", "full"):
        lab, n = ndimage.label(CC.masks(shape)[name])
        lab = np.ascontiguousarray(lab, np.int32)
        table = np.empty((n + 1, 7), np.uint64)
        native.ia3cpu_label_sums(_p(lab), *shape, n, _p(table))
        cen, cnt = R.label_centers(lab, n)
        assert np.array_equal(table[1:, 0].astype(np.int64), cnt)
        with np.errstate(invalid="ignore", divide="ignore"):
            got = table[1:, 1::2].astype(np.float64) / table[1:, 2::2].astype(np.float64)
        assert got.tobytes() == cen.tobytes(), name
        for l in (1, n):   # the per-label statement is the reference's function on label == l
            assert np.array_equal(R.binary_center(lab == l), cen[l - 1], equal_nan=True)


# ---- rules pinned against the installed SciPy / NumPy --------------------------------------------------------------------------
def test_even_window_reads_minus_two_to_plus_one(native):
    x = np.zeros(16)
    x[8] = 1.0
    for s, lo, hi in ((1, 0, 0), (2, -1, 0), (3, -1, 1), (4, -2, 1), (5, -2, 2)):
        w = (C.c_int * 3)()
        native.ia3cpu_window(s, w)
        assert (w[0], w[1]) == (lo, hi) and w[2] == int(np.ceil(s / 2))
        hit = np.nonzero(ndimage.maximum_filter(x, s, mode='nearest'))[0]
        # output i reads inputs i + lo .. i + hi, so the impulse at 8 shows at 8 - hi .. 8 - lo
        assert hit.tolist() == list(range(8 - hi, 8 - lo + 1)), s
        assert np.array_equal(ndimage.minimum_filter(-x, s, mode='nearest'), -ndimage.maximum_filter(x, s, mode='nearest'))
    y = np.arange(6.)[::-1].copy()
    assert ndimage.maximum_filter(y, 4, mode='nearest').tolist() == [5, 5, 5, 4, 3, 2]   # indices clamped at both ends


def test_threshold_compare_is_strict_and_in_float64():
    th = np.float64(np.float32(0.1)) + 1e-12          # between float32(0.1) and the next float32
    seed = np.array([np.float32(0.1), np.nextafter(np.float32(0.1), np.float32(1))], dtype=np.float32)
    assert type(th) is np.float64 and (seed > th).tolist() == [False, True]
    assert (seed > np.float32(th)).tolist() == [False, True] and (seed.astype(np.float64) > th).tolist() == [False, True]
    assert not (seed[:1] > np.float64(seed[0])).any()                      # strict
    # a float64 scalar is not demoted to the array's float32: the compare sees th itself, not float32(th)
    th2 = np.float64(seed[1]) - 1e-12
    assert np.float32(th2) == seed[1] and (seed > th2).tolist() == [False, True]
    from scipy.stats import scoreatpercentile
    assert type(scoreatpercentile(seed, 50)) is np.float64


def test_centres_average_the_indices_above_zero(gold):
    m = _center_rule_mask()
    c = R.binary_center(m)
    assert c.tolist() == [1.0, 1.5, 2.0] and np.array_equal(c, gold["center_rule"])   # not [0.5, 1.0, 1.5]
    inds = np.indices(m.shape).astype(np.uint16)
    assert (inds * m).dtype == np.uint16 and np.mean((inds[2] * m)[(inds[2] * m) > 0]).dtype == np.float64
    with np.errstate(invalid="ignore"), pytest.warns(RuntimeWarning):
        assert np.isnan(np.mean(np.zeros(0, np.uint16)))
    # plane medians: float64 for uint16 (mean of the two middle values), float32 arithmetic for float32
    assert np.median(np.array([[1, 2], [4, 9]], np.uint16)) == 3.0 and type(np.median(np.ones((2, 2), np.uint16))) is np.float64
    f = np.array([[1, 16777216], [16777218, 3e7]], np.float32)
    assert type(np.median(f)) is np.float32 and np.median(f) == (f[0, 1] + f[1, 0]) / np.float32(2)
    assert (f / np.median(f)).dtype == np.float32 and (np.ones((2, 2), np.uint16) / np.median(f.astype(np.uint16))).dtype == np.float64


# ---- the shim ------------------------------------------------------------------------------------------------------------------
SIGNATURES = {
    "find_candidate_chromosomes": [("_chrom_im", E), ("_adjust_layers", False), ("_filt_size", 3), ("_binary_per_th", 99.5),
                                   ("_morphology_size", 1), ("_min_label_size", 100), ("_random_walk_beta", 10),
                                   ("_num_threads", 12), ("_verbose", True), ("_return_label", False)],
    "_calculate_binary_center": [("_binary_label", E)],
    "find_candidate_chromosomes_in_nucleus": [("_chrom_im", E), ("_dna_im", E), ("_dna_mask", None), ("_chr_seed_size", 200),
                                              ("_filt_size", 3), ("_num_of_iter", 10), ("_percent_th_3chr", 97.5),
                                              ("_percent_th_2chr", 85), ("_use_percent_chr_area", False), ("_fold_3chr", 6),
                                              ("_fold_2chr", 4), ("_std_ratio", 3), ("_morphology_size", 1),
                                              ("_min_label_size", 30), ("_random_walk_beta", 15), ("_num_threads", 4),
                                              ("_verbose", True)],
    "select_candidate_chromosomes": [("_cand_chrom_coords", E), ("_spots_list", E), ("_cand_spot_intensity_th", 0.5),
                                     ("_good_chr_loss_th", 0.4), ("_verbose", True)],
    "identify_chromosomes": [("chrom_im", E), ("dapi_im", None), ("seed_gfilt_size", 0.75), ("background_gfilt_size", 7.5),
                             ("chrom_snr_th", 1.5), ("dapi_snr_th", 2), ("morphology_size", 1), ("min_label_size", 25),
                             ("num_threads", 12), ("return_seed_im", False), ("verbose", True)],
}


def test_names_and_signatures():
    from imageanalysis3_amd.segmentation_tools import chromosome as CH
    for name, want in SIGNATURES.items():
        got = [(p.name, p.default) for p in inspect.signature(getattr(CH, name)).parameters.values()]
        assert got == want, (name, got)
    from imageanalysis3_amd.segmentation_tools import morphology as M
    for name in ("ball", "binary_erosion", "binary_dilation", "binary_closing", "binary_fill_holes", "label",
                 "remove_small_objects", "label_centers"):
        assert callable(getattr(M, name))


def test_signatures_equal_the_reference_source_where_it_is_present():
    import ref_loader
    ref = os.path.join(ref_loader.REF, "segmentation_tools", "chromosome.py")
    if not os.path.isfile(ref):
        return   # the table above is the record; this only guards it where the reference tree is at hand
    import ast
    defs = {n.name: n for n in ast.parse(open(ref).read()).body if isinstance(n, ast.FunctionDef)}
    for name, want in SIGNATURES.items():
        a = defs[name].args
        names = [x.arg for x in a.args]
        defaults = [E] * (len(names) - len(a.defaults)) + [ast.literal_eval(x) for x in a.defaults]
        mine = [w for w in want if w[0] != "_return_label"]
        assert list(zip(names, defaults)) == mine, name


def test_ctypes_mirror_of_the_parameter_struct(tmp_path):
    from imageanalysis3_amd import _lib
    lines = ['printf("%zu", sizeof(ia3_chrom_params));']
    for f in _lib.ChromParams._fields_:
        lines.append('printf(" %%zu", offsetof(ia3_chrom_params, %s));' % f[0])
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ia3.h"\nint main(void){%s return 0;}\n' % "".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(HERE, "..", "include"), str(src), "-o", str(exe)])
    tok = subprocess.check_output([str(exe)]).decode().split()
    assert int(tok[0]) == C.sizeof(_lib.ChromParams)
    for f, off in zip(_lib.ChromParams._fields_, tok[1:]):
        assert getattr(_lib.ChromParams, f[0]).offset == int(off), f[0]


def test_argument_errors_before_the_device(monkeypatch):
    from imageanalysis3_amd import _lib
    from imageanalysis3_amd.segmentation_tools import chromosome as CH
    from imageanalysis3_amd.segmentation_tools import morphology as M

    def no_device(*a, **k):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(_lib.DeviceStack, "upload", classmethod(no_device))
    monkeypatch.setattr(_lib, "lib", no_device)
    im = CC.generated("small", "u16")
    zero = im.copy()
    zero[3, :, :40] = 0                        # more than half of plane 3
    with pytest.raises(ValueError, match="plane 3"):
        CH.find_candidate_chromosomes(zero, _verbose=False)
    bad = im.astype(np.float32)
    bad[5, 0, 0] = np.nan
    with pytest.raises(ValueError, match="plane 5"):
        CH.find_candidate_chromosomes(bad, _verbose=False)
    for fs in (0, 6, 3.5):
        with pytest.raises(NotImplementedError, match="_filt_size"):
            CH.find_candidate_chromosomes(im, _filt_size=fs, _verbose=False)
    with pytest.raises(NotImplementedError, match="_morphology_size"):
        CH.find_candidate_chromosomes(im, _morphology_size=2, _verbose=False)
    f64 = im.astype(np.float64)
    f64[0, 0, 0] += 1e-9
    with pytest.raises(NotImplementedError, match="exact in float32"):
        CH.find_candidate_chromosomes(f64, _verbose=False)
    with pytest.raises(IndexError):
        CH.find_candidate_chromosomes(im[0], _verbose=False)
    with pytest.raises(TypeError):
        CH.find_candidate_chromosomes(im.astype(np.int64), _verbose=False)
    for f in (CH.find_candidate_chromosomes_in_nucleus, CH.identify_chromosomes):
        with pytest.raises(NotImplementedError, match="binary_fill_holes"):
            f(im, im)
    with pytest.raises(NotImplementedError, match="spot_tools.picking"):
        CH.select_candidate_chromosomes([], [])
    m = np.zeros((4, 4, 4), bool)
    with pytest.raises(NotImplementedError):
        M.binary_erosion(m, M.ball(3))
    with pytest.raises(NotImplementedError):
        M.binary_dilation(m, np.ones((3, 3, 3)))          # 26-connected
    with pytest.raises(NotImplementedError):
        M.binary_fill_holes(m, M.ball(2))
    with pytest.raises(TypeError):
        M.binary_closing(m.astype(np.float32))
    with pytest.raises(IndexError):
        M.label(m[0])
