"""Inputs and NumPy restatement of the illumination-profile generator (csrc/stats.hip, correction_tools/illumination.py).

The fixture tests/golden/illum.npz (scripts/make_illum_golden.py) holds only what the reference's own
``_image_to_profile`` and ``Generate_illumination_correction`` returned; the inputs are regenerated here.  The
restatement spells out the arithmetic the device code reproduces bit for bit:

  scoreatpercentile   idx = per / 100. * (n - 1); the order statistic idx when that is whole, else
                      (s[i] * w0 + s[i + 1] * w1) / (w0 + w1) with w0 = i + 1 - idx, w1 = idx - i, in float64
  clip and sum        each voxel min(max(float64(v), lo), hi); planes added in z order, starting from plane 0
  Gaussian            float64, axis 0 then axis 1, np_oracle.correlate1d's summation order, mode reflect
  across images       sum in image order / N, the same Gaussian, divided by its maximum
"""
import os

import numpy as np

import np_oracle as O

CAPS = ([5, 90], [90, 5], [0.5, 99.9])
SIGMAS = (3, 60)
STACK_SHAPES = ((5, 24, 40), (12, 64, 96))
MOVIE_NAMES = ("Conv_zscan_2.dax", "Conv_zscan_10.dax", "Conv_zscan_1.dax")   # used in the order 1, 2, 10
MOVIE_CHANNELS = ['750', '561']
MOVIE_SIGMA = 10
HOT_COLUMN_561 = (33, 12, 15000)


def prepared_stacks():
    """The uint16 channel stacks of fixture (a): spots on a background with a smooth illumination fall-off, a few
    saturated and zero voxels."""
    from imageanalysis3_amd import synth
    out = []
    for k, shape in enumerate(STACK_SHAPES):
        im = synth.make_fov(shape, 5 + 3 * k, 70 + k, dtype=np.float32, margin=(1, 4, 4))[0].astype(np.float64)
        x, y = np.meshgrid(np.arange(shape[1]), np.arange(shape[2]), indexing="ij")
        fall = 1.0 - 0.5 * (((x - 0.45 * shape[1]) / shape[1]) ** 2 + ((y - 0.55 * shape[2]) / shape[2]) ** 2)
        im = np.clip(im * fall[None] * 9.7, 0, 65535).astype(np.uint16)   # spread out: few ties around the cap ranks
        im[0, 0, :3] = 65535
        im[-1, -1, -2:] = 0
        out.append(im)
    return out


def profile_cases():
    """(key, stack index, remove_cap, cap_th_per, sigma) of fixture (a)."""
    cases = []
    for s in range(len(STACK_SHAPES)):
        for sigma in SIGMAS:
            for c, cap in enumerate(CAPS):
                cases.append(("prof_s%d_sig%d_cap%d" % (s, sigma, c), s, True, list(cap), sigma))
            cases.append(("prof_s%d_sig%d_nocap" % (s, sigma), s, False, [5, 90], sigma))
    return cases


def movies():
    """Three 4-colour 12 x 64 x 64 movies (raw (frames, X, Y) uint16) made from the correction-chain case: another
    brightness and fall-off per movie, and one more hot column in the 561 channel only.  Returns (case, [raw, ...])."""
    from conftest import build_chain_case
    case = build_chain_case()
    Z, X, Y, nb = case["Z"], case["X"], case["Y"], case["nb"]
    x, y = np.meshgrid(np.arange(X), np.arange(Y), indexing="ij")
    raws = []
    for k in range(3):
        fall = 1.0 - (0.3 + 0.1 * k) * (((x - (24 + 6 * k)) / X) ** 2 + ((y - (36 - 4 * k)) / Y) ** 2)
        raw = np.clip(case["raw"].astype(np.float64) * (1.0 + 0.15 * k) * fall[None] + 11 * k, 0, 65535).astype(np.uint16)
        start = nb + (case["chs"].index('561') - nb) % 4
        hx, hy, hv = HOT_COLUMN_561
        raw[start:start + Z * 4:4, hx, hy] = hv
        raws.append(raw)
    return case, raws


def write_movies(folder):
    """The movies as .dax files in ``folder``; returns the chain case."""
    from conftest import write_dax
    case, raws = movies()
    for name, raw in zip(MOVIE_NAMES, raws):
        write_dax(os.path.join(folder, name), raw)
    return case


def movie_kwargs(case, z_shift_corr):
    return dict(sel_channels=list(MOVIE_CHANNELS), single_im_size=[case["Z"], case["X"], case["Y"]],
                all_channels=case["chs"], num_buffer_frames=case["nb"], num_empty_frames=0, z_shift_corr=z_shift_corr,
                gaussian_filter_size=MOVIE_SIGMA, parallel=False, make_plot=False, verbose=False)


# ---- the restatement -------------------------------------------------------------------------------------------

def score_at_percentile(a, per):
    s = np.sort(np.asarray(a).ravel())
    idx = per / 100. * (s.size - 1)
    i = int(idx)
    if i == idx:
        return np.float64(s[i])
    w0, w1 = i + 1 - idx, idx - i
    return (np.float64(s[i]) * w0 + np.float64(s[i + 1]) * w1) / (w0 + w1)


def clip_sum_z(im, limits=None):
    """Sum over z of the float64 voxels, clamped to ``limits`` = (lo, hi) when given; planes in z order."""
    acc = None
    for plane in np.asarray(im):
        p = plane.astype(np.float64)
        if limits is not None:
            p = np.minimum(np.maximum(p, limits[0]), limits[1])
        acc = p if acc is None else acc + p
    return acc


def gaussian_f64(im, sigma, truncate=4.0, mode="reflect"):
    w, _ = O.gaussian_kernel1d(sigma, truncate)
    out = np.asarray(im, dtype=np.float64)
    for ax in (0, 1):
        out = O.correlate1d(out, w, ax, mode)
    return out


def cap_limits(im, cap_th_per):
    lims = [score_at_percentile(im, min(cap_th_per)), score_at_percentile(im, max(cap_th_per))]
    return min(lims), max(lims)


def image_profile(im, remove_cap=True, cap_th_per=(5, 90), sigma=40):
    limits = cap_limits(im, cap_th_per) if remove_cap else None
    return gaussian_f64(clip_sum_z(im, limits), sigma)


def combine_profiles(profiles, sigma):
    """Profiles of one channel, one per image in image order -> the normalised profile."""
    acc = profiles[0]
    for p in profiles[1:]:
        acc = acc + p
    pf = gaussian_f64(acc / len(profiles), sigma)
    return pf / np.max(pf)


def generate(raws, case, z_shift_corr, hot_pixel_corr=True, hot_pixel_th=4, remove_cap=True, cap_th_per=(5, 90)):
    """Generate_illumination_correction on in-memory movies (in processing order), through np_oracle's restatement of
    the pre-correction chain.  Returns the list of profiles in the order of MOVIE_CHANNELS."""
    size = [case["Z"], case["X"], case["Y"]]
    per_image = []
    for raw in raws:
        ims = O.correct_fov_image(raw, MOVIE_CHANNELS, size, case["chs"], num_buffer_frames=case["nb"],
                                  corr_channels=MOVIE_CHANNELS, hot_pixel_corr=hot_pixel_corr, hot_pixel_th=hot_pixel_th,
                                  z_shift_corr=z_shift_corr, illumination_corr=False, bleed_corr=False,
                                  chromatic_corr=False, verbose=False)
        per_image.append([image_profile(im, remove_cap, cap_th_per, MOVIE_SIGMA) for im in ims])
    return [combine_profiles([r[i] for r in per_image], MOVIE_SIGMA) for i in range(len(MOVIE_CHANNELS))]


def movies_in_order():
    """(case, raws sorted the way the driver sorts the files: by the integer after the last '_')."""
    case, raws = movies()
    order = sorted(range(len(MOVIE_NAMES)), key=lambda k: int(MOVIE_NAMES[k].split('.dax')[0].split('_')[-1]))
    return case, [raws[k] for k in order]
