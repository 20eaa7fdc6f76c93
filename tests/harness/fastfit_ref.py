"""NumPy statement of the fast path of ``External/Fitting_v4.py`` that fastfit.hip implements: box-normalised
seeds (``get_seed_points_base_v2``) and closed-form moment fits (``gfit_fast`` / ``fast_fit_big_image``).

Written from the description of the arithmetic, one NumPy operation per step, so that every
rounding happens where the reference's happens; tests/test_fastfit_cpu.py holds it to the reference's own output
(tests/golden/fastfit.npz) bit for bit.  The GPU machine has no reference: device tests on other inputs compare
with this file.  The box blur is tests/harness/blur_ref.py's (OpenCV is not installed where this project is built).
"""
import numpy as np

from . import blur_ref


def normalise(im, sz=20):
    """float32 stack minus its sz x sz box blur, plane by plane."""
    im32 = np.asarray(im).astype(np.float32)
    return im32 - np.stack([blur_ref.box_blur(plane, sz) for plane in im32])


def seeds(im, gfilt_size=5, filt_size=3, th_seed=3., max_num=None, std=None):
    """(centers_zxyh, std_).  ``std``: use this value instead of ``np.std`` of the stack (the device's value, which
    differs from NumPy's float32 result in the last bits) so that the voxel tests can be compared exactly."""
    stack = normalise(im, gfilt_size) if gfilt_size != 0 else np.asarray(im)
    std_ = np.std(stack) if std is None else std
    cutoff = std_ * th_seed
    pix = int(filt_size / 2)
    keep = (stack > cutoff) & (stack > 0)
    for dz in range(-pix, pix + 1):
        for dx in range(-pix, pix + 1):
            for dy in range(-pix, pix + 1):
                # np.roll by -d: position p sees the value at (p + d) modulo the shape
                keep &= stack >= np.roll(stack, (-dz, -dx, -dy), axis=(0, 1, 2))
    z, x, y = np.nonzero(keep)
    h = stack[z, x, y]
    order = np.argsort(h, kind="stable")[::-1]
    out = np.array([z[order], x[order], y[order], h[order]])
    if max_num is not None:
        out = out[:, :max_num]
    return out, std_


def ball_offsets(radius):
    """(n, 3) integer offsets in [-radius, radius) per axis with d^2 <= radius^2, z-major order."""
    r = int(radius)
    g = np.arange(-r, r)
    off = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    return off[(off * off).sum(1) <= r * r]


def moments(values, coords, bk_f=0.1):
    """The twelve numbers of gfit_fast for voxel values (n,) and integer coordinates (3, n)."""
    values = np.asarray(values)
    coords = np.ascontiguousarray(coords)    # as the reference builds it: NumPy's pairwise order needs a contiguous axis
    n = len(values)
    if n == 0:
        return np.full(12, np.nan)
    bk = np.sort(values)[int(n * bk_f)]
    w = values - bk                      # in the image's dtype: uint16 wraps
    w[w < 0] = 0
    h = np.max(w)
    with np.errstate(invalid="ignore", divide="ignore"):
        w = w / np.sum(w)                # all weights zero: 0 / 0, NaN moments, as the reference gives
    centre = np.sum(coords * w, -1)      # integer times weight in float64, NumPy's pairwise order
    dev = coords - centre[:, None]       # (3, n) float64
    cov = {}
    for i in range(3):
        for j in range(i, 3):
            cov[i, j] = np.sum(np.ascontiguousarray(dev[i] * dev[j] * w))
    return np.array([h, centre[0], centre[1], centre[2], bk, cov[0, 0], cov[1, 1], cov[2, 2], cov[0, 1], cov[0, 2],
                     cov[1, 2], np.nan])


def voxel_sets(im, centers, radius_fit=4, avoid_neigbors=True, recenter=False):
    """Per centre the (values, coords (3, n)) the fast fit works on."""
    im = np.asarray(im)
    centers = np.asarray(centers)
    shape = np.array(im.shape)
    off = ball_offsets(radius_fit)
    c64 = centers.astype(np.float64)
    out = []
    for i, c in enumerate(centers):
        mine = off
        if avoid_neigbors:
            diff = c64 - c64[i]
            near = np.nonzero(np.sqrt((diff * diff).sum(1)) <= 2 * radius_fit)[0]    # ascending, self included
            rel = c64[near] - c64[i]
            d = rel[:, None, :] - off[None, :, :].astype(np.float64)
            sq = d * d
            dist = np.sqrt((sq[..., 0] + sq[..., 1]) + sq[..., 2])     # cdist: squares added in axis order, sqrt
            mine = off[near[np.argmin(dist, 0)] == i]                  # first minimum = lowest seed index
        base = np.array([int(v) for v in c])
        for _ in range(2 if recenter else 1):
            pos = base + mine
            pos = pos[np.all((pos >= 0) & (pos < shape), 1)]
            vals = im[pos[:, 0], pos[:, 1], pos[:, 2]]
            if len(vals) == 0:
                break
            base = pos[np.argmax(vals)]
        out.append((vals, np.ascontiguousarray(pos.T)))       # (3, n) C order: the sums run over a contiguous axis
    return out


def fast_fit(im, centers, radius_fit=4, avoid_neigbors=True, recenter=False, bk_f=0.1):
    """(N, 12) float64 rows of fast_fit_big_image(better_fit=False); shape (0,) for no centres."""
    sets = voxel_sets(im, centers, radius_fit, avoid_neigbors, recenter)
    return np.array([moments(v, x, bk_f) for v, x in sets])
