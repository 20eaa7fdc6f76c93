"""GPU: the drift measurement off its defaults.  phase_cross_correlation and align_image (csrc/fft_align.hip, the crop loop
and rule of csrc/movie.cpp) against scikit-image 0.18.3 / the reference's align_image (tests/golden/phase_edges.npz) and
against the NumPy oracle, at the sizes where the arithmetic branches.  Which test reaches which branch:

  half_power_k / half_combine_k, odd Y (no Nyquist column, inner = (Y-1)/2)   ..vs_golden_and_oracle[odd, yodd, tiles]
  the mirror (Z-kz)%Z, (X-kx)%X at odd Z, X                                   ..vs_golden_and_oracle[odd, zxodd, tiles]
  complex route, Y < 8                                                        ..vs_golden_and_oracle[short], crop rule[cy7]
  wrap rule dims/2 at odd and even sizes, at and past half an axis            test_whole_voxel_rolls
  an axis of length 1                                                         ..vs_golden_and_oracle[unit]
  both contractions and both transform forms against an independent answer   test_odd_shapes_on_the_other_routes
  crop_to_real_k's unaligned rows, half_power2_k at odd Y, batched            crop rule[odd_crops]
  drift_crops falling back: unequal crops / short rows / upsample 1           crop rule[mixed_crops, cy7, mg*_pf1]
  first batch of 1, 2, 3, 3 crops; tail after the batch ending with flag 0    crop rule[mg*_pf*, four_*]
  consensus / closest_three in C++ with 1, 2, 4, 8 drifts                     crop rule[one_crop, two_crops, four_*, ..]
  more than eight crops                                                       crop rule[nine_crops, nine_crops_all]

A case is compared only where the oracle's peak is no near-tie; test_align_edges_cpu.py asserts that of every case here.
"""
import contextlib
import ctypes as C
import functools
import io
import re
import numpy as np
import pytest
from conftest import load_golden
import np_oracle as O
import align_edge_cases as E
from align_edge_cases import SHIFT_ATOL, assert_record

pytestmark = pytest.mark.gpu

NORMS = (None, "phase")


@pytest.fixture(scope="module")
def golden():
    return load_golden("phase_edges.npz")


@functools.lru_cache(maxsize=None)
def oracle_pcc(name, tag, up, norm):
    a, b = E.pcc_pair(name, dict(E.DTYPES)[tag])
    return O.phase_cross_correlation(a, b, upsample_factor=up, normalization=norm)


def _check_case(name, golden, with_golden):
    from imageanalysis3_amd import _lib as L
    from imageanalysis3_amd.correction_tools.alignment import phase_cross_correlation
    shape = E.PCC_CASES[name][0]
    for tag, dt in E.DTYPES:
        a, b = E.pcc_pair(name, dt)
        with L.DeviceStack.upload(a) as da, L.DeviceStack.upload(b) as db:
            for up in E.UPSAMPLES:
                for norm in NORMS:
                    so, eo, po = oracle_pcc(name, tag, up, norm)
                    for where, x, y in (("host", a, b), ("resident", da, db)):
                        got = phase_cross_correlation(x, y, upsample_factor=up, normalization=norm)
                        what = (name, tag, up, norm, where)
                        assert_record(got, np.concatenate([so, [eo, po]]), what + ("oracle",))
                        if norm is None and with_golden:
                            assert_record(got, golden[E.pcc_key(name, tag, up)], what + ("scikit-image",))
                        for ax in range(3):
                            if shape[ax] == 1:
                                assert got[0][ax] == 0, what


@pytest.mark.parametrize("name", list(E.PCC_CASES))
def test_phase_cross_correlation_vs_golden_and_oracle(golden, name):
    _check_case(name, golden, True)


@pytest.mark.parametrize("tune", ["IA3_TUNE_DFT_VALU", "IA3_TUNE_FFT_C2C"])
@pytest.mark.parametrize("name", list(E.ODD_CASES))
def test_odd_shapes_on_the_other_routes(golden, name, tune):
    """The vector-unit contraction and the complex transforms, each against the oracle and the library's answer rather
    than against its twin."""
    from imageanalysis3_amd import _lib as L
    try:
        L.check(L.lib().ia3_set_tuning(getattr(L, tune), C.c_int(1)))
        _check_case(name, golden, True)
    finally:
        L.check(L.lib().ia3_set_tuning(L.IA3_TUNE_DFT_VALU, C.c_int(0)))
        L.check(L.lib().ia3_set_tuning(L.IA3_TUNE_FFT_C2C, C.c_int(0)))


@pytest.mark.parametrize("name", list(E.ROLL_CASES))
def test_whole_voxel_rolls(golden, name):
    """np.roll(ref, r) against ref: the shift is -r folded by np.fix(size / 2), exactly."""
    from imageanalysis3_amd import _lib as L
    from imageanalysis3_amd.correction_tools.alignment import phase_cross_correlation
    for k in range(len(E.ROLL_CASES[name][4])):
        want = E.roll_expected(name, k)
        for tag, dt in E.DTYPES:
            a, b = E.roll_pair(name, k, dt)
            with L.DeviceStack.upload(a) as da, L.DeviceStack.upload(b) as db:
                for up in E.ROLL_UPSAMPLES:
                    for norm in NORMS:
                        for where, x, y in (("host", a, b), ("resident", da, db)):
                            got = phase_cross_correlation(x, y, upsample_factor=up, normalization=norm)
                            what = (name, k, tag, up, norm, where)
                            assert np.array_equal(got[0], want), what + (got[0], want)
                            if norm is None:
                                assert_record(got, golden[E.roll_key(name, k, tag, up)], what, exact_error=0.)


def test_argument_edges():
    from imageanalysis3_amd import _lib as L
    from imageanalysis3_amd.correction_tools.alignment import phase_cross_correlation
    a, b = E.pcc_pair("odd", np.float32)
    with L.DeviceStack.upload(a) as da, L.DeviceStack.upload(b) as db, L.DeviceStack.upload(b[:, :-1]) as dc:
        for x, y in ((a, b), (da, db)):
            with pytest.raises(ValueError):
                phase_cross_correlation(x, y, upsample_factor=0)
            with pytest.raises(ValueError):
                phase_cross_correlation(x, y, upsample_factor=10, normalization="amplitude")
        with pytest.raises(ValueError):
            phase_cross_correlation(a, b[:, :-1], upsample_factor=10)
        with pytest.raises(ValueError):
            phase_cross_correlation(da, dc, upsample_factor=10)
    # a float32 reference with a uint16 moving image: the moving image is taken to float32
    b16 = b.astype(np.uint16)
    for up in (1, 100):
        for norm in NORMS:
            mixed = phase_cross_correlation(a, b16, upsample_factor=up, normalization=norm)
            both = phase_cross_correlation(a, b16.astype(np.float32), upsample_factor=up, normalization=norm)
            assert np.array_equal(mixed[0], both[0]) and mixed[1:] == both[1:], (up, norm, mixed, both)
            so, eo, po = O.phase_cross_correlation(a, b16, upsample_factor=up, normalization=norm)
            assert_record(mixed, np.concatenate([so, [eo, po]]), (up, norm))


# ---- the crop loop and the rule ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_crop_shift(image, tag, crop, fold, norm):   # (the cases share most of their crops)
    src, ref = E.align_images(image, dict(E.DTYPES)[tag])
    s = tuple(slice(crop[2 * a], crop[2 * a + 1]) for a in range(3))
    return O.phase_cross_correlation(ref[s], src[s], upsample_factor=fold, normalization=norm)[0]


def oracle_align(name, tag, norm):
    """np_oracle.align_image — consensus_drift over its per-crop phase correlations — on the clipped crop list;
    returns (drift, flag, crops used)."""
    image, crops, kw = E.align_cases()[name]
    used = []

    def per_crop():
        for c in E.clip_crops(crops):
            used.append(1)
            yield _oracle_crop_shift(image, tag, tuple(int(v) for v in c.ravel()), kw.get("precision_fold", 100), norm)
    d, f = O.consensus_drift(per_crop(), kw.get("min_good_drifts", 3), kw.get("drift_diff_th", 1.))
    return d, f, len(used)


def _align(A, *args, **kw):
    """align_image with verbose=True: (drift, flag, the N of its "-- N crops in" line)."""
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        d, f = A.align_image(*args, use_autocorr=True, verbose=True, **kw)
    n = re.findall(r"^-- (\d+) crops in", out.getvalue(), re.M)
    assert len(n) == 1, out.getvalue()
    return d, f, int(n[0])


@pytest.mark.parametrize("name", list(E.align_cases()))
def test_align_image_crop_rule(golden, monkeypatch, name):
    from imageanalysis3_amd import _lib as L
    from imageanalysis3_amd.correction_tools import alignment as A
    image, crops, kw = E.align_cases()[name]
    n_crops = len(crops)
    for tag, dt in E.DTYPES:
        src, ref = E.align_images(image, dt)
        for norm in NORMS:
            monkeypatch.setattr(A, "DEFAULT_NORMALIZATION", norm)
            want, wflag, wn = oracle_align(name, tag, norm)
            what = (name, tag, norm)
            if name.startswith("four_"):
                assert (wflag, wn) == (0, 4), what        # the property of the oracle this case is built for
            if name in ("one_crop", "two_crops"):
                assert (wflag, wn) == (1, n_crops), what
            runs = [("host", _align(A, src, ref, crop_list=crops, **kw))]
            if n_crops <= A.MAX_DEVICE_CROPS:
                with L.DeviceStack.upload(src) as ds:
                    dref = A.DriftReference(ref, crop_list=crops, dtype=dt)
                    try:
                        runs.append(("reference spectra", _align(A, ds, dref, **kw)))
                    finally:
                        dref.free()
            else:
                with pytest.raises(ValueError, match="at most 8 crops"):
                    A.DriftReference(ref, crop_list=crops, dtype=dt)
                with L.DeviceStack.upload(src) as ds, L.DeviceStack.upload(ref) as dr:
                    runs.append(("resident", _align(A, ds, dr, crop_list=crops, **kw)))
            for where, (d, f, n) in runs:
                assert f == wflag and n == wn, what + (where, f, wflag, n, wn)
                assert np.allclose(d, want, rtol=0, atol=SHIFT_ATOL), what + (where, d, want)
                if norm is None:
                    exp = golden[E.align_key(name, tag)]
                    assert f == int(exp[3]), what + (where,)
                    assert np.allclose(d, exp[:3], rtol=0, atol=SHIFT_ATOL), what + (where, d, exp[:3])
