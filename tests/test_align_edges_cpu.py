"""CPU: the oracle's phase correlation and align_image against what scikit-image 0.18.3 and the reference's align_image
answer off the friendly sizes (tests/golden/phase_edges.npz, recorded by oracle/make_golden_h5.py phase_edges), the
condition under which those cases may be compared at all (no near-tie at the peak), and the Python consensus rule on
designed drift lists.  test_gpu_align_edges.py holds the device to the same file and the same oracle."""
import functools
import warnings
import numpy as np
import pytest
from conftest import load_golden
import np_oracle as O
import align_edge_cases as E
from align_edge_cases import SHIFT_ATOL, MIN_GAP, assert_record


@pytest.fixture(scope="module")
def golden():
    return load_golden("phase_edges.npz")


def test_golden_is_the_real_library(golden):
    assert str(golden["skimage_version"]) == "0.18.3"


@pytest.mark.parametrize("name", list(E.PCC_CASES))
def test_oracle_phase_correlation_vs_scikit_image_off_the_friendly_sizes(golden, name):
    shape = E.PCC_CASES[name][0]
    for tag, dt in E.DTYPES:
        a, b = E.pcc_pair(name, dt)
        assert a.shape == shape
        for up in E.UPSAMPLES:
            for norm in (None, "phase"):
                gaps = E.peak_gaps(a, b, up, norm)
                assert min(gaps) >= MIN_GAP, (name, tag, up, norm, gaps)
            got = O.phase_cross_correlation(a, b, upsample_factor=up, normalization=None)
            assert_record(got, golden[E.pcc_key(name, tag, up)], (name, tag, up))
            for ax in range(3):
                if shape[ax] == 1:
                    assert got[0][ax] == 0 and golden[E.pcc_key(name, tag, up)][ax] == 0


@pytest.mark.parametrize("name", list(E.ROLL_CASES))
def test_oracle_whole_voxel_rolls_and_the_wrap_rule(golden, name):
    for k in range(len(E.ROLL_CASES[name][4])):
        want = E.roll_expected(name, k)
        for tag, dt in E.DTYPES:
            a, b = E.roll_pair(name, k, dt)
            for up in E.ROLL_UPSAMPLES:
                exp = golden[E.roll_key(name, k, tag, up)]
                assert np.array_equal(exp[:3], want), (name, k, tag, up, exp[:3], want)
                for norm in (None, "phase"):
                    assert min(E.peak_gaps(a, b, up, norm)) >= MIN_GAP, (name, k, tag, up, norm)
                    s, e, p = O.phase_cross_correlation(a, b, upsample_factor=up, normalization=norm)
                    assert np.array_equal(s, want), (name, k, tag, up, norm, s, want)
                    if norm is None:
                        assert_record((s, e, p), exp, (name, k, tag, up), exact_error=0.)


def test_wrap_rule_at_half_an_axis():
    """np.fix(size / 2): half an even axis comes back positive, an odd axis has no such point."""
    assert np.array_equal(E.roll_expected("even", 1), [4, 16, 23])
    assert np.array_equal(E.roll_expected("odd", 1), [-3, -16, -22])
    assert np.array_equal(E.roll_expected("odd", 2), [3, 16, 22])


def _oracle_align(name, dt, norm):
    """(drift, flag, crops used) of the oracle on an align_image case."""
    image, crops, kw = E.align_cases()[name]
    src, ref = E.align_images(image, dt)
    cl = E.clip_crops(crops)
    used = []
    real = O.phase_cross_correlation

    def counting(*a, **k):
        used.append(1)
        return real(*a, **k)
    O.phase_cross_correlation = counting
    try:
        d, f = O.align_image(src, ref, crop_list=cl, use_autocorr=True, normalization=norm, **kw)
    finally:
        O.phase_cross_correlation = real
    return d, f, len(used)


@functools.lru_cache(maxsize=None)
def _crop_gaps(image, tag, crop, fold, norm):   # (many cases share the default crops)
    src, ref = E.align_images(image, dict(E.DTYPES)[tag])
    s = tuple(slice(crop[2 * a], crop[2 * a + 1]) for a in range(3))
    return tuple(E.peak_gaps(ref[s], src[s], fold, norm))


@pytest.mark.parametrize("name", list(E.align_cases()))
def test_oracle_align_image_vs_reference_crop_rule(golden, name):
    image, crops, kw = E.align_cases()[name]
    for tag, dt in E.DTYPES:
        src, ref = E.align_images(image, dt)
        for c in E.clip_crops(crops):
            for norm in (None, "phase"):
                gaps = _crop_gaps(image, tag, tuple(c.ravel()), kw.get("precision_fold", 100), norm)
                assert min(gaps) >= MIN_GAP, (name, tag, c.tolist(), norm, gaps)
        d, f, n = _oracle_align(name, dt, None)
        exp = golden[E.align_key(name, tag)]
        assert f == int(exp[3]), (name, tag, f, exp)
        assert np.allclose(d, exp[:3], rtol=0, atol=SHIFT_ATOL), (name, tag, d, exp)


def test_designed_cases_reach_what_they_are_for():
    """The properties the device tests lean on, stated of the oracle: a first batch of 1, 2, 3, 3 crops is enough for
    min_good_drifts 1 .. 4 up to the fourth crop; the rolled source meets the rule at the fourth crop exactly; one and
    two crops end in the closest-three rule; nine crops can all be needed."""
    for mg, n_want in ((1, 1), (2, 2), (3, 3), (4, 4)):
        for pf in (1, 10, 100):
            d, f, n = _oracle_align("mg%d_pf%d" % (mg, pf), np.uint16, None)
            assert (f, n) == (0, n_want), (mg, pf, f, n)
    for k in (0, 1, 2):
        for tag, dt in E.DTYPES:
            for norm in (None, "phase"):
                d, f, n = _oracle_align("four_%d" % k, dt, norm)
                assert (f, n) == (0, 4), (k, tag, norm, f, n)
    for name, n_want in (("one_crop", 1), ("two_crops", 2), ("nine_crops_all", 9)):
        for norm in (None, "phase"):
            d, f, n = _oracle_align(name, np.float32, norm)
            assert (f, n) == (1, n_want), (name, norm, f, n)
    sizes = {tuple(np.diff(c, axis=1).ravel()) for c in E.align_cases()["mixed_crops"][1][:3]}
    assert len(sizes) == 3
    assert all(tuple(np.diff(c, axis=1).ravel()) == (11, 31, 33) for c in E.align_cases()["odd_crops"][1])
    assert any(c[2][1] - c[2][0] == 7 for c in E.align_cases()["cy7"][1])
    assert (E.align_cases()["beyond"][1][:, :, 1] > np.array(E.ALIGN_SHAPE)).any()


def _python_rule(drifts, min_good_drifts, drift_diff_th):
    """align_image's use of _consensus_drift after every crop and _closest_three_drift at the end."""
    from imageanalysis3_amd.correction_tools.alignment import _consensus_drift, _closest_three_drift
    for n in range(1, len(drifts) + 1):
        d, _ = _consensus_drift(drifts[:n], min_good_drifts, drift_diff_th)
        if d is not None:
            return d, 0, n
    return _closest_three_drift(drifts), 1, len(drifts)


RULE_CASES = {
    # two pairs equally close: the first in row-major order wins, the third is the drift nearest to both
    "tie": ([(0., 0., 0.), (3., 0., 0.), (0., 3., 0.), (10., 10., 10.), (3., 3., 0.)], 3, 1.),
    # two rows: the pair and, again, its first member
    "two_rows": ([(0., 0., 0.), (5., 1., 0.)], 3, 1.),
    # a NaN component: that crop is never "close", nanmean skips it
    "nan": ([(0., np.nan, 0.), (0.25, 2., 0.), (0., 2.25, 0.25), (0.5, 2., 0.)], 3, 1.),
    "nan_no_agreement": ([(0., np.nan, 0.), (0.25, 2., 0.), (9., 2.25, 0.25)], 3, 1.),
    # distances of exactly drift_diff_th count as agreement (<=)
    "at_threshold": ([(0., 0., 0.), (2., 0., 0.), (1., 0., 0.)], 3, 1.),
    "just_past_threshold": ([(0., 0., 0.), (2., 0., 0.), (1., 0., 0.)], 3, np.nextafter(1., 0.)),
    "min_good_1": ([(4., 5., 6.), (0., 0., 0.)], 1, 1.),
    # an outlier drags the mean away: the rule is met only by the fifth drift
    "min_good_2_late": ([(0., 0., 0.), (5., 0., 0.), (0.5, 0., 0.), (0.25, 0., 0.), (0.3, 0., 0.)], 2, 1.),
}


@pytest.mark.parametrize("name", list(RULE_CASES))
def test_python_consensus_rule_vs_oracle(name):
    drifts, mg, th = RULE_CASES[name]
    drifts = [np.array(d) for d in drifts]
    seen = []

    def feed():
        for d in drifts:
            seen.append(1)
            yield d
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)   # nanmean over a column that is all NaN so far
        want, wf = O.consensus_drift(feed(), mg, th)
        got, gf, n = _python_rule(drifts, mg, th)
    assert gf == wf and n == len(seen), (name, gf, wf, n, len(seen))
    assert np.array_equal(got, want, equal_nan=True), (name, got, want)


def test_rule_cases_end_where_they_are_meant_to():
    ends = {}
    for name, (drifts, mg, th) in RULE_CASES.items():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            ends[name] = _python_rule([np.array(d) for d in drifts], mg, th)[1:]
    assert ends == {"tie": (1, 5), "two_rows": (1, 2), "nan": (0, 4), "nan_no_agreement": (1, 3), "at_threshold": (0, 3),
                    "just_past_threshold": (1, 3), "min_good_1": (0, 1), "min_good_2_late": (0, 5)}
