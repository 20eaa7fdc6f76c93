"""TEST INFRASTRUCTURE — NumPy / SciPy statement of ``find_candidate_chromosomes`` (reference:
segmentation_tools/chromosome.py:264-361) and of the five scikit-image functions it calls, which is not installed where
these tests run (INTEGRATION.md §2 has the precedent, ``cv2.blur``).  scripts/make_chromosome_golden.py runs the
reference's own function with these five functions standing in for ``skimage`` and stores its outputs in
tests/golden/chromosome.npz; a deployment that has scikit-image can compare the five against the real ones.

Nothing here is shipped; nothing here runs on the GPU.
"""
import warnings

import numpy as np
from scipy import ndimage
from scipy.stats import scoreatpercentile


# ---- scikit-image ------------------------------------------------------------------------------------------------------------
def ball(radius, dtype=np.uint8):
    """skimage.morphology.ball: 1 where dz^2 + dx^2 + dy^2 <= radius^2 in a (2 radius + 1)^3 array."""
    z, x, y = np.mgrid[-radius:radius + 1, -radius:radius + 1, -radius:radius + 1]
    return np.array(z * z + x * x + y * y <= radius * radius, dtype=dtype)


def closing(image, footprint):
    """skimage.morphology.closing of a bool image: dilation, where the outside adds nothing, then erosion, where the
    outside takes nothing away (for ball(1) scikit-image's 'reflect' border is the same thing: a voxel mirrored across a
    face lands on the voxel itself, which the footprint holds anyway)."""
    d = ndimage.binary_dilation(image, footprint, border_value=0)
    return ndimage.binary_erosion(d, footprint, border_value=1)


def opening(image, footprint):
    """skimage.morphology.opening of a bool image: erosion, then dilation, with the same border rule."""
    e = ndimage.binary_erosion(image, footprint, border_value=1)
    return ndimage.binary_dilation(e, footprint, border_value=0)


def remove_small_objects(ar, min_size=64):
    """skimage.morphology.remove_small_objects: a bool array is labelled first (connectivity 1); objects of fewer than
    min_size voxels become 0, the other labels stay."""
    out = ar.copy()
    if min_size == 0:
        return out
    if out.dtype == bool:
        ccs = ndimage.label(ar, ndimage.generate_binary_structure(ar.ndim, 1))[0]
    else:
        ccs = out
    sizes = np.bincount(ccs.ravel())
    too_small = sizes < min_size
    out[too_small[ccs]] = 0
    return out


def random_walker(data, labels, beta=130, mode='cg_j', **kwargs):
    """skimage.segmentation.random_walker where it has nothing to do: "Random walker only segments unlabeled areas, where
    labels == 0. No zero valued areas in labels were found. Returning provided labels." """
    if (labels != 0).all():
        warnings.warn('Random walker only segments unlabeled areas, where labels == 0. No zero valued areas in labels '
                      'were found. Returning provided labels.', stacklevel=2)
        return labels
    raise NotImplementedError("the random walk itself is not stated here: find_candidate_chromosomes never reaches it")


# ---- the chain ---------------------------------------------------------------------------------------------------------------
def binary_center(binary_label):
    """chromosome.py:4-10"""
    inds = np.indices(np.shape(binary_label)).astype(np.uint16)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return np.array([np.mean(l[l > 0]) for l in (inds * binary_label)])


def label_centers(labels, max_label):
    """(centres (max_label, 3), counts (max_label,)) of the labels 1..max_label, one ``binary_center`` each."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        cen = np.full((max_label, 3), np.mean(np.zeros(0, np.uint16)))   # a label that does not occur: the mean of nothing
    cnt = np.bincount(labels.ravel().astype(np.int64), minlength=max_label + 1)[1:max_label + 1].astype(np.int64)
    inds_all = np.indices(labels.shape).astype(np.uint16)
    for obj, sl in enumerate(ndimage.find_objects(labels.astype(np.int32), max_label)):
        if sl is None:
            continue
        inds = inds_all[(slice(None),) + sl]   # the box of the object: voxels outside it add nothing to either sum
        sub = labels[sl] == obj + 1
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            cen[obj] = [np.mean(l[l > 0]) for l in (inds * sub)]
    return cen, cnt


def chain(im, filt_size=3, binary_per_th=99.5, morphology_size=1, min_label_size=100):
    """Every stage of find_candidate_chromosomes on ``im``: dict with medians, seed, threshold, binary, opened, filled,
    closed, label, n, kept_label (uint16), sizes (of the kept labels), coords."""
    r = {}
    r["medians"] = [np.median(lyr) for lyr in im]
    adj = np.array([lyr / np.median(lyr) for lyr in im])
    seed = ndimage.maximum_filter(adj, filt_size, mode='nearest') - ndimage.minimum_filter(adj, filt_size, mode='nearest')
    r["seed"] = seed
    r["threshold"] = scoreatpercentile(seed, binary_per_th)
    b = seed > r["threshold"]
    e = int(np.ceil(filt_size / 2))
    b[:e] = 0
    b[-e:] = 0
    b[:, :e] = 0
    b[:, -e:] = 0
    b[:, :, :e] = 0
    b[:, :, -e:] = 0
    r["binary"] = b.copy()
    fp = ball(morphology_size)
    o = ndimage.binary_dilation(ndimage.binary_erosion(b, fp), fp)
    r["opened"] = o
    f = ndimage.binary_fill_holes(o, structure=fp)
    r["filled"] = f
    c = closing(opening(f, ball(0)), ball(1))
    r["closed"] = c
    lab, n = ndimage.label(c)
    r["label"], r["n"] = lab.copy(), n
    lab[lab == 0] = -1
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        seg = random_walker(adj, lab, beta=10, mode='cg_mg')
    seg[seg < 0] = 0
    kept = remove_small_objects(seg, min_label_size).astype(np.uint16)
    r["kept_label"] = kept
    ids = np.unique(kept)
    ids = ids[ids > 0]
    r["ids"] = ids
    r["sizes"] = np.array([(kept == i).sum() for i in ids], dtype=np.int64)
    r["coords"] = np.array([binary_center(kept == i) for i in ids])
    return r
