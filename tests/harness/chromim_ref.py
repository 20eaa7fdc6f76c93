"""TEST INFRASTRUCTURE — NumPy / SciPy statement of the chromosome image (reference: classes/field_of_view.py:1853-1901,
the loop body of ``Field_of_View._generate_chrom_im_from_data``): both paths, written as the reference orders them.
``background`` stands in for ``find_image_background`` on the slow path (the tests hand in the package's own, which has
its own tests).

Nothing here is shipped; nothing here runs on the GPU.
"""
import numpy as np
from scipy import ndimage


def fast_add(acc, im, flag, drift):
    """:1871-1891 for one image; ``drift`` is the rounded one."""
    if flag == 2:
        acc += im
        return
    drift = np.asarray(drift)
    llim = np.max([drift, np.zeros(len(drift), dtype=int)], axis=0)
    shift_llim = np.max([-drift, np.zeros(len(drift), dtype=int)], axis=0)
    rlim = np.array(np.shape(im)) - shift_llim
    shift_rlim = shift_llim + (rlim - llim)
    crops = tuple(slice(l, r) for l, r in zip(llim, rlim))
    shift_crops = tuple(slice(l, r) for l, r in zip(shift_llim, shift_rlim))
    background = np.median(im)
    acc += background
    acc[shift_crops] += im[crops] - background


def chrom_im(ims, flags, drifts, single_im_size, fast=True, background=None, acc=None):
    """The float64 image.  ``acc``: a sum to go on from."""
    acc = np.zeros(single_im_size) if acc is None else acc
    if fast:
        rough = np.round(drifts).astype(int) if len(ims) else []
        for im, flag, drift in zip(ims, flags, rough):
            fast_add(acc, im, flag, drift)
    else:
        for im, flag, drift in zip(ims, flags, drifts):
            if flag == 2:
                shifted = im
            else:
                shifted = ndimage.shift(im, -np.asarray(drift), order=1, mode='constant', cval=background(im))
            acc += shifted
    return acc


def shifted_sum(ims, flags, drifts, single_im_size):
    """The fast path stated the other way round: per image the moved copy filled up with the median, added in reversed
    order."""
    acc = np.zeros(single_im_size)
    rough = np.round(drifts).astype(int)
    Z, X, Y = single_im_size
    z, x, y = np.meshgrid(np.arange(Z), np.arange(X), np.arange(Y), indexing="ij")
    for im, flag, d in list(zip(ims, flags, rough))[::-1]:
        if flag == 2:
            acc += im
            continue
        sz, sx, sy = z + d[0], x + d[1], y + d[2]
        inside = (sz >= 0) & (sz < Z) & (sx >= 0) & (sx < X) & (sy >= 0) & (sy < Y)
        moved = np.full(single_im_size, np.median(im))
        moved[inside] = im[sz[inside], sx[inside], sy[inside]]
        acc += moved
    return acc
