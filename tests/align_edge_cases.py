"""Inputs of the drift-measurement edge tests (test_align_edges_cpu.py, test_gpu_align_edges.py) and of the recipe that
records what the real library answers for them (oracle/make_golden_h5.py phase_edges -> tests/golden/phase_edges.npz).

Nothing here touches the device: the stacks come from imageanalysis3_amd.synth with fixed arguments, so the golden file
holds results only.  The three users import the same tables, so a case cannot drift apart from its recorded answer.
"""
import functools
import numpy as np

UPSAMPLES = (1, 2, 3, 7, 10, 100)
DTYPES = (("f32", np.float32), ("u16", np.uint16))

# name -> (shape, beads, seed, drift injected into the moving image, margin); what each shape reaches:
PCC_CASES = {
    "odd":    ((7, 33, 45), 8, 3, (0.6, -2.3, 3.45), (1, 4, 4)),       # all axes odd
    "yodd":   ((8, 32, 47), 8, 5, (-0.7, 1.75, -4.2), (1, 4, 4)),      # only Y odd: no Nyquist column
    "zxodd":  ((9, 31, 40), 8, 7, (1.3, -3.6, 2.15), (1, 4, 4)),       # Z and X odd: the mirror (Z-kz)%Z, (X-kx)%X
    "short":  ((6, 40, 7), 5, 11, (0.4, 2.7, -0.8), (1, 4, 1)),        # row shorter than 8: complex transforms
    "unit":   ((1, 48, 50), 10, 13, (0.0, -2.4, 3.3), (0, 5, 5)),      # an axis of length 1: shift 0 along it
    "tiles":  ((13, 70, 121), 12, 3, (-1.31, 2.77, -0.46), (3, 10, 10)),   # no multiple of the matrix-core tiles
}
ODD_CASES = ("odd", "yodd", "zxodd", "tiles")   # shapes with an odd axis on the real-input route

# whole-voxel rolls of one bead image: nothing, half of every axis, half plus one, mixed signs beyond half
ROLL_CASES = {
    "odd":  ((7, 33, 45), 8, 3, (1, 4, 4), ((0, 0, 0), (3, 16, 22), (4, 17, 23), (-5, 20, -30))),
    "even": ((8, 32, 46), 8, 5, (1, 4, 4), ((0, 0, 0), (4, 16, 23), (5, 17, 24), (-6, 19, -29))),
}
ROLL_UPSAMPLES = (1, 10)

ALIGN_SHAPE = (12, 128, 128)
ALIGN_DRIFT = (0.4, -2.3, 3.1)


@functools.lru_cache(maxsize=None)
def _pcc_pair_f32(name):
    from imageanalysis3_amd import synth
    shape, nb, seed, drift, margin = PCC_CASES[name]
    ref, src, _, _ = synth.make_bead_pair(shape, nb, seed, np.array(drift), margin=margin, min_sep=4.0)
    ref.setflags(write=False); src.setflags(write=False)
    return ref, src


def pcc_pair(name, dtype):
    """(reference, moving) of a PCC case in `dtype` (uint16: the float32 stack truncated, as phase.npz does)."""
    ref, src = _pcc_pair_f32(name)
    return ref.astype(dtype), src.astype(dtype)


def pcc_key(name, tag, up):
    return "pcc_%s_%s_%d" % (name, tag, up)


@functools.lru_cache(maxsize=None)
def _roll_ref_f32(name):
    from imageanalysis3_amd import synth
    shape, nb, seed, margin, _ = ROLL_CASES[name]
    ref, _, _, _ = synth.make_bead_pair(shape, nb, seed, np.zeros(3), margin=margin, min_sep=4.0)
    ref.setflags(write=False)
    return ref


def roll_pair(name, k, dtype):
    ref = _roll_ref_f32(name).astype(dtype)
    return ref, np.roll(ref, ROLL_CASES[name][4][k], axis=(0, 1, 2))


def roll_key(name, k, tag, up):
    return "roll_%s_%d_%s_%d" % (name, k, tag, up)


def roll_expected(name, k):
    """The shift that registers np.roll(ref, r) onto ref: -r folded into the range the wrap rule keeps,
    (-size/2, size/2] for an even axis, [-(size-1)/2, (size-1)/2] for an odd one (np.fix(size / 2))."""
    shape, r = ROLL_CASES[name][0], ROLL_CASES[name][4][k]
    out = []
    for n, v in zip(shape, r):
        e = (-v) % n
        out.append(float(e - n if e > n // 2 else e))
    return np.array(out)


# ---- align_image: the crop loop and the consensus rule -----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _align_pair_f32():
    from imageanalysis3_amd import synth
    ref, src, _, _ = synth.make_bead_pair(ALIGN_SHAPE, 90, 17, np.array(ALIGN_DRIFT), margin=(2, 6, 6), min_sep=6.0)
    ref.setflags(write=False); src.setflags(write=False)
    return ref, src


def default_crops():
    """generate_drift_crops((12, 128, 128)): eight 12 x 32 x 32 crops (restated: the recipe runs without the package's
    library)."""
    cts = [(32, 32), (96, 96), (96, 32), (32, 96), (64, 32), (64, 96), (32, 64), (96, 64)]
    return np.array([[[0, 12], [x - 16, x + 16], [y - 16, y + 16]] for x, y in cts])


def four_crop_pair(k, dtype):
    """A source that is the reference rolled by (0, 2, -3) except inside crop k, where it is the reference rolled by
    (0, 2, -1): crop k measures a drift 2 px off in y, so the rule is satisfied by the fourth crop and not before."""
    ref = _align_pair_f32()[0].astype(dtype)
    src = np.roll(ref, (0, 2, -3), axis=(0, 1, 2))
    bad = np.roll(ref, (0, 2, -1), axis=(0, 1, 2))
    s = tuple(slice(a, b) for a, b in default_crops()[k])
    src[s] = bad[s]
    return src, ref


def _odd_crops():      # 11 x 31 x 33: odd rows (unaligned stores of the crop copy) and odd-Y spectra, batched
    return np.array([[[0, 11], [x, x + 31], [y, y + 33]] for x, y in ((3, 5), (70, 11), (40, 80), (90, 90), (9, 60))])


def _mixed_crops():    # three sizes in the first batch: the batched route hands over to the per-crop one
    return np.array([[[0, 12], [8, 40], [8, 40]], [[1, 12], [60, 91], [20, 53]], [[0, 10], [30, 70], [70, 118]],
                     [[0, 12], [80, 112], [80, 112]]])


def _cy7_crops():      # a crop whose rows are 7 long among ordinary ones
    return np.array([[[0, 12], [16, 48], [30, 37]], [[0, 12], [16, 48], [16, 48]], [[0, 12], [80, 112], [16, 48]],
                     [[0, 12], [80, 112], [80, 112]], [[0, 12], [48, 80], [80, 112]]])


def _beyond_crops():   # upper limits past the image: Python slicing and alignment.py:254-256 both clip them
    return np.array([[[0, 20], [100, 140], [96, 128]], [[2, 14], [16, 48], [100, 150]], [[0, 12], [90, 128], [10, 42]],
                     [[0, 12], [48, 80], [48, 80]]])


def nine_crops():
    return np.concatenate([default_crops(), np.array([[[0, 12], [48, 80], [48, 80]]])])


def clip_crops(crops, shape=ALIGN_SHAPE):
    c = np.array(crops, dtype=int).reshape(-1, 3, 2).copy()
    c[:, :, 0] = np.maximum(c[:, :, 0], 0)
    c[:, :, 1] = np.minimum(c[:, :, 1], np.array(shape)[None, :])
    return c


def align_cases():
    """name -> (image, crop_list, keyword arguments).  image: "pair" (sub-voxel drift everywhere) or ("four", k)."""
    cases = {}
    for mg in (1, 2, 3, 4):
        for pf in (1, 10, 100):
            cases["mg%d_pf%d" % (mg, pf)] = ("pair", default_crops(), dict(min_good_drifts=mg, precision_fold=pf))
    for k in (0, 1, 2):
        cases["four_%d" % k] = (("four", k), default_crops(), {})
    cases["odd_crops"] = ("pair", _odd_crops(), {})
    cases["mixed_crops"] = ("pair", _mixed_crops(), {})
    cases["cy7"] = ("pair", _cy7_crops(), {})
    cases["one_crop"] = ("pair", default_crops()[:1], {})
    cases["two_crops"] = ("pair", default_crops()[:2], {})
    cases["nested_lists"] = ("pair", default_crops()[2:6].tolist(), {})
    cases["beyond"] = ("pair", _beyond_crops(), {})
    cases["nine_crops"] = ("pair", nine_crops(), {})
    cases["nine_crops_all"] = ("pair", nine_crops(), dict(drift_diff_th=0.))   # no three agree exactly: all nine are used
    return cases


def align_images(image, dtype):
    """(src, ref) of an align_image case."""
    if image == "pair":
        ref, src = _align_pair_f32()
        return src.astype(dtype), ref.astype(dtype)
    return four_crop_pair(image[1], dtype)


def align_key(name, tag):
    return "align_%s_%s" % (name, tag)


# ---- how a result is compared -------------------------------------------------------------------------------------
SHIFT_ATOL = 1e-9     # the bars of test_phase_correlation_and_align_image_vs_scikit_image_golden
SCALAR_ATOL = 1e-5
MIN_GAP = 1e-9        # relative gap between the two largest |values| below which a peak counts as a near-tie


def circle_diff(a, b):
    """|a - b| on the circle: a negative real peak may come out as +pi or -pi."""
    return abs((a - b + np.pi) % (2 * np.pi) - np.pi)


def assert_record(got, exp, what, exact_error=None):
    """(shift, error, phasediff) against a recorded [shift, error, phasediff].
    `exact_error`: the error is known in closed form (0 for a rolled copy) and takes the place of the recorded one.
    There the library's own figure is sqrt(|1 - q|) with q = 1 up to rounding, in single precision for float32 input
    (7e-4 recorded, 3e-8 for the same stack as uint16): the exact value is the stricter reference at the same bar."""
    s, e, p = got
    assert np.allclose(s, exp[:3], rtol=0, atol=SHIFT_ATOL), (what, s, exp[:3])
    e_ref = exp[3] if exact_error is None else exact_error
    assert abs(e - e_ref) <= SCALAR_ATOL, (what, e, e_ref)
    assert circle_diff(p, exp[4]) <= SCALAR_ATOL, (what, p, exp[4])


# ---- the condition under which a case may be compared at all ------------------------------------------------------
def peak_gaps(reference_image, moving_image, upsample_factor, normalization):
    """Relative gap between the largest and the second largest |value| of the coarse correlation and (upsample > 1) of
    the upsampled grid, as np_oracle.phase_cross_correlation computes them.  A unit axis is left out of the upsampled
    grid: the grid is constant along it and the shift there is defined as 0."""
    import np_oracle as O
    src = np.fft.fftn(np.asarray(reference_image, dtype=np.float64))
    tgt = np.fft.fftn(np.asarray(moving_image, dtype=np.float64))
    prod = src * tgt.conj()
    if normalization == "phase":
        prod /= np.maximum(np.abs(prod), 100 * np.finfo(np.float64).eps)
    cc = np.fft.ifftn(prod)

    def gap(a):
        v = np.sort(np.abs(a).ravel())
        return (v[-1] - v[-2]) / v[-1] if len(v) > 1 else 1.0
    gaps = [gap(cc)]
    if upsample_factor > 1:
        shape = np.array(cc.shape)
        peak = np.array(np.unravel_index(np.argmax(np.abs(cc)), cc.shape), dtype=np.float64)
        mid = np.fix(shape / 2)
        peak[peak > mid] -= shape[peak > mid]
        uf = float(upsample_factor)
        peak = np.round(peak * uf) / uf
        region = int(np.ceil(uf * 1.5))
        up = O._upsampled_dft(prod.conj(), region, uf, np.fix(region / 2.0) - peak * uf)
        up = up[tuple(slice(0, 1) if n == 1 else slice(None) for n in cc.shape)]
        gaps.append(gap(up))
    return gaps
