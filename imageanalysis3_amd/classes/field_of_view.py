"""Flat forms of ``Field_of_View`` methods (reference: classes/field_of_view.py), as ``classes.preprocess.
fit_spots_by_segmentation`` is the flat form of a ``DaxProcesser`` method.  The class itself stays the reference's: there
is no ``Field_of_View`` here.

``generate_chrom_im`` / ``generate_chrom_im_from_data`` are ``Field_of_View._generate_chrom_im_from_data`` (:1821-1917),
the chromosome image of an experiment without a chromosome stain: the float64 sum of every processed round, the unwarped
ones moved by their drift.  The sum is kept on the device (``_lib.ChromImage``, csrc/chromim.hip) and
``segmentation_tools.chromosome.find_candidate_chromosomes`` takes it from there, bit for bit with the reference.

``select_chromosome_by_candidate_spots`` is ``Field_of_View._select_chromosome_by_candidate_spots`` (:2273-2339): the
candidates that keep a spot in enough rounds (csrc/select.hip).

All ``file:line`` citations are relative to the reference tree.
"""
import time

import numpy as np

from . import _allowed_kwds
from .. import _lib as L


def _check_images(ims, flags, drifts, shape):
    """The argument checks of ``generate_chrom_im``, all before the device is touched: (flags, drifts as an (n, 3) array
    of the dtype given)."""
    ims = list(ims)
    n = len(ims)
    flags = [int(f) for f in flags]
    drifts = np.asarray(drifts) if n else np.zeros((0, 3))
    if len(flags) != n or len(drifts) != n:
        raise ValueError("generate_chrom_im: %d images, %d flags, %d drifts" % (n, len(flags), len(drifts)))
    if n and (drifts.ndim != 2 or drifts.shape[1] != 3):
        raise ValueError("drifts should be an (n, 3) table of z, x, y, got shape %s" % (drifts.shape,))
    for k, im in enumerate(ims):
        if not isinstance(im, (np.ndarray, L.DeviceStack)):
            raise TypeError("image %d should be a numpy.ndarray or a resident DeviceStack, but %s is given." % (k, type(im)))
        if np.dtype(im.dtype) != np.uint16:
            raise NotImplementedError("image %d is %s: the chromosome image is built from uint16 images (what a save file "
                                      "holds; with float32 values the sums are no longer order-free)" % (k, im.dtype))
        if tuple(im.shape) != shape:
            raise IndexError("image %d has the shape %s, the chromosome image %s" % (k, tuple(im.shape), shape))
    return ims, flags, drifts


def _rounded_shifts(flags, drifts, shape):
    """:1870 ``np.round(_drifts).astype(np.int)`` (half to even, on the dtype given) and NumPy's refusal of the two crops
    of :1883-1891 when a shift reaches the length of its axis."""
    rough = np.round(drifts).astype(int).reshape(-1, 3)
    for k, (flag, d) in enumerate(zip(flags, rough)):
        if flag == 2:
            continue
        for axis in range(3):
            if abs(int(d[axis])) >= shape[axis]:
                lhs = [max(shape[a] - abs(int(d[a])), 0) for a in range(3)]
                raise ValueError("image %d: operands could not be broadcast together: the rounded drift %s reaches the "
                                 "image size %s (remaining crop %s)" % (k, d.tolist(), list(shape), lhs))
    return rough


def _add_warped(chrom, stack, drift):
    """:1900-1901 — ``shift(im, -drift, order=1, mode='constant', cval=find_image_background(im))`` is
    ``map_coordinates(im, grid + drift, ...)`` in every byte: the order-1 constant warp, added as it is."""
    from ..io_tools.load import find_image_background
    cval = find_image_background(stack)
    minus = np.ascontiguousarray(-np.asarray(drift, dtype=np.float64))   # the warp reads at grid - drift
    with L.DeviceStack.empty(stack.shape, np.uint16) as shifted:
        L.check(L.lib().ia3_warp3d_dev(stack._h, L.dptr(minus), None, 0, 1, L.MODE_CONSTANT, float(cval), shifted._h))
        chrom.add([shifted], [2], [[0, 0, 0]])


def generate_chrom_im(ims, flags, drifts, single_im_size=None, fast=True, chrom_im=None, return_device=False):
    """classes/field_of_view.py:1853-1901 — the loop body of ``_generate_chrom_im_from_data`` for images that are at
    hand: ``ims`` uint16 ndarrays and / or resident ``DeviceStack``s (never downloaded), ``flags`` what the save file
    holds for them (2: warped, added as it is; otherwise moved by the drift), ``drifts`` (n, 3).

    ``fast`` (``_fast``): the drift is rounded (``np.round(drifts).astype(int)``), voxels the moved image does not cover
    get its ``np.median``; ``|round(drift)|`` of an axis length or more is the ``ValueError`` NumPy raises there.
    ``fast=False``: ``scipy.ndimage.shift(im, -drift, order=1, mode='constant', cval=find_image_background(im))``.
    ``single_im_size``: the image size (default: that of ``chrom_im``, else of the first image).  ``chrom_im``: a
    ``ChromImage`` to go on adding to (the sum is exact, so batches may come in any split).  Returns the float64 ndarray,
    or with ``return_device=True`` the resident ``ChromImage`` (``chrom_im`` itself when one was given)."""
    ims = list(ims)
    if chrom_im is not None and not isinstance(chrom_im, L.ChromImage):
        raise TypeError("chrom_im should be a ChromImage, but %s is given." % type(chrom_im))
    if single_im_size is not None:
        shape = tuple(int(v) for v in single_im_size)
    elif chrom_im is not None:
        shape = tuple(chrom_im.shape)
    elif ims and hasattr(ims[0], "shape"):
        shape = tuple(ims[0].shape)
    elif ims:
        raise TypeError("image 0 should be a numpy.ndarray or a resident DeviceStack, but %s is given." % type(ims[0]))
    else:
        raise ValueError("single_im_size is required when there is no image")
    if len(shape) != 3:
        raise IndexError("a 3-D (z,x,y) image size is required, got %s" % (shape,))
    if chrom_im is not None and tuple(chrom_im.shape) != shape:
        raise IndexError("chrom_im has the shape %s, single_im_size is %s" % (tuple(chrom_im.shape), shape))
    ims, flags, drifts = _check_images(ims, flags, drifts, shape)
    shifts = _rounded_shifts(flags, drifts, shape) if fast else None
    chrom = chrom_im if chrom_im is not None else L.ChromImage.empty(shape)
    try:
        # host images are resident one launch's worth at a time
        for first in range(0, len(ims), L.CHROM_ADD_BATCH):
            idx = range(first, min(first + L.CHROM_ADD_BATCH, len(ims)))
            mine, stacks = [], []
            try:
                for k in idx:
                    if isinstance(ims[k], L.DeviceStack):
                        stacks.append(ims[k])
                    else:
                        stacks.append(L.DeviceStack.upload(ims[k]))
                        mine.append(stacks[-1])
                if fast:
                    chrom.add(stacks, [flags[k] for k in idx], shifts[first:first + len(stacks)])
                else:
                    for k, s in zip(idx, stacks):
                        if flags[k] == 2:
                            chrom.add([s], [2], [[0, 0, 0]])
                        else:
                            _add_warped(chrom, s, drifts[k])
            finally:
                for s in mine:
                    s.free()
        if return_device:
            return chrom
        out = chrom.download()
    except Exception:
        if chrom_im is None:
            chrom.free()
        raise
    if chrom_im is None:
        chrom.free()
    return out


def generate_chrom_im_from_data(save_filename, data_type, num_loaded_image=10, fast=True, image_dtype=np.uint16,
                                return_device=False, verbose=True):
    """classes/field_of_view.py:1821-1917 ``Field_of_View._generate_chrom_im_from_data`` on a FOV save file: every id of
    the ``data_type`` group whose flag is > 0, in file order, loaded ``num_loaded_image`` at a time and added up on the
    device.  Returns the float64 chromosome image, or the resident ``ChromImage`` with ``return_device=True``.  Keeping it
    as an attribute and writing it into the save file are the caller's."""
    from .batch_functions import SaveFile, load_image_from_fov_file, _require_file
    if data_type not in _allowed_kwds:
        raise ValueError(f"Wrong input data_type: {data_type}, should be among:{_allowed_kwds}")
    if np.dtype(image_dtype) != np.uint16:
        raise NotImplementedError("image_dtype %s: the chromosome image is built from uint16 images" % np.dtype(image_dtype))
    num_loaded_image = int(num_loaded_image)
    if num_loaded_image < 1:
        raise ValueError("num_loaded_image should be at least 1")
    _require_file(save_filename, "save")
    with SaveFile(save_filename, data_type) as sf:
        all_flags = np.asarray(sf['flags'][...])
        valid_ids = np.asarray(sf['ids'][...])[all_flags > 0]   # only load from processed ids
        shape = tuple(int(v) for v in sf['ims'].shape[1:])
    if verbose:
        print(f"- Generate chromosome image from {data_type} images, {len(valid_ids)} images planned to load.")
        chrom_time = time.time()
    chrom = L.ChromImage.empty(shape)
    try:
        for batch in range(int(np.ceil(len(valid_ids) / num_loaded_image))):
            load_ids = valid_ids[batch * num_loaded_image:(batch + 1) * num_loaded_image]
            ims, flags, drifts = load_image_from_fov_file(save_filename, data_type, load_ids, image_dtype=image_dtype,
                                                          load_drift=True, verbose=verbose)
            if verbose:
                print(f"-- shifting images", end=' ')
                shift_time = time.time()
            generate_chrom_im(ims, flags, drifts, single_im_size=shape, fast=fast, chrom_im=chrom, return_device=True)
            if verbose:
                print(f"in {time.time()-shift_time:.3f}s. ")
        if verbose:
            print(f"-- finish generating chrom_im in {time.time()-chrom_time:.3f}s. ")
        if return_device:
            return chrom
        out = chrom.download()
    except Exception:
        chrom.free()
        raise
    chrom.free()
    return out


def select_chromosome_by_candidate_spots(spots_list, cand_chrom_coords, _good_chr_loss_th=0.4, _cand_spot_intensity_th=0.5,
                                         _verbose=True, return_info=False):
    """classes/field_of_view.py:2273-2339 ``Field_of_View._select_chromosome_by_candidate_spots`` on the spot tables of
    every round (the ``{spot_type}_spots_list`` attribute) and the candidate centres (``cand_chrom_coords``): the
    ``chrom_coords`` array of ``segmentation_tools.chromosome.select_candidate_chromosomes`` (:2325).  Loading the two from
    the save file, keeping the result as an attribute and saving it are the caller's.

    ``return_info=True``: ``(chrom_coords, removed, lost, chrom_spots)`` with the original indices of the removed candidates
    in removal order, the rounds without a spot per candidate (at its removal for a removed one) and, per kept chromosome,
    what ``spot_tools.picking.assign_spots_to_chromosomes`` gives it of every round's selected spots, taken from the owners
    the device already holds.  ``lost`` and ``chrom_spots`` are None where the reference returns every candidate without
    looking at a spot (``_good_chr_loss_th >= 1``, no rounds)."""
    from ..segmentation_tools.chromosome import _select_chromosomes
    from ..spot_tools.picking import split_rows_by_owner
    _cand_chrom_coords = list(cand_chrom_coords)
    _chrom_coords, info = _select_chromosomes(_cand_chrom_coords, spots_list, _cand_spot_intensity_th, _good_chr_loss_th,
                                              _verbose, owners=return_info)
    if not return_info:
        return _chrom_coords
    chrom_spots = None
    if info["lost"] is not None:
        chrom_spots = [[] for _ in _chrom_coords]
        for sel, own in zip(info["sels"], info["owner"]):
            per = split_rows_by_owner(sel, own, len(_chrom_coords)) if len(sel) else [[] for _ in _chrom_coords]
            for i, rows in enumerate(per):
                chrom_spots[i].append(rows)
    return _chrom_coords, info["removed"], info["lost"], chrom_spots
