"""Neighbourhood boxes around fitted spots (interface of the reference's io_tools/crop.py:59-152)."""
import numpy as np
from .. import _image_size
from .. import _lib as L


def generate_neighboring_crop(coord, crop_size=5, single_im_size=_image_size, sub_pixel_precision=False):
    """``ImageCrop`` covering ``coord - crop_size .. coord + crop_size`` (inclusive) on every axis, clipped to the
    image; limits are rounded to whole pixels unless ``sub_pixel_precision`` (the int32 box then truncates them)."""
    from ..classes.preprocess import ImageCrop
    size = np.asarray(single_im_size)
    nd = len(size)
    half = np.broadcast_to(np.asarray(crop_size), (nd,)) if np.ndim(crop_size) == 0 else np.asarray(crop_size)[:nd]
    centre = np.asarray(coord)[:nd]
    lo, hi = centre - half, centre + half + 1
    if not sub_pixel_precision:
        lo, hi = np.round(lo), np.round(hi)
    box = np.stack([np.maximum(lo, 0), np.minimum(hi, size.astype(np.int32))], axis=1)
    return ImageCrop(nd, box, single_im_size=single_im_size)


def _box_sizes(crop_sizes, dim=3):
    """crop.py:127-130 — per-axis box sizes from an int or a list / ndarray; checked against what the kernel is built for."""
    if isinstance(crop_sizes, (int, np.integer)) and not isinstance(crop_sizes, bool):
        _sizes = np.ones(dim, dtype=np.int32) * int(crop_sizes)
    elif isinstance(crop_sizes, (list, np.ndarray)):
        _sizes = np.array(crop_sizes)[:dim]
        if len(_sizes) != dim or not np.all(_sizes == np.floor(_sizes)):
            raise ValueError(f"crop_sizes should give {dim} whole numbers, got {crop_sizes}")
        _sizes = _sizes.astype(np.int32)
    else:
        raise TypeError(f"wrong input crop_sizes, should be int, list or np.ndarray, but {type(crop_sizes)} is given")
    if np.any(_sizes < 1) or np.any(_sizes > L.CROP_MAX):
        raise ValueError(f"crop sizes should be between 1 and {L.CROP_MAX}, got {_sizes}")
    return _sizes


def crop_neighboring_areas(im, centers, crop_sizes):
    """``np.array([crop_neighboring_area(im, c, crop_sizes) for c in centers])`` in one device call: (n, cz, cx, cy) of
    the image's dtype.  ``im``: a (Z,X,Y) uint16 / float32 ndarray (uploaded for the call) or a resident ``DeviceStack``."""
    if not isinstance(im, (np.ndarray, L.DeviceStack)):
        raise TypeError("wrong input image, should be np.ndarray")
    _sizes = _box_sizes(crop_sizes)
    _centers = np.array(centers, dtype=np.float64)
    if _centers.ndim != 2 or _centers.shape[1] < 3:
        raise ValueError("centers should be n rows of (z, x, y)")
    _centers = np.ascontiguousarray(_centers[:, :3])
    _resident = isinstance(im, L.DeviceStack)
    _stack = im if _resident else L.DeviceStack.upload(im)
    try:
        return L.crop_pairs(_stack, _centers, _sizes)[0]
    finally:
        if not _resident:
            _stack.free()


def crop_neighboring_area(im, center, crop_sizes, extrapolate_mode='nearest'):
    """crop.py:107-152 — the box of ``crop_sizes`` voxels centred on the sub-pixel ``center``: a rough crop around it,
    then ``map_coordinates`` (cubic, mode 'nearest') at ``center + (idx - (crop - 1) / 2)``; same values as the reference,
    in the image's dtype.  Runs on the device (``ia3_crop_pairs_dev``); ``im`` may be a resident ``DeviceStack``.  Only
    the reference's default ``extrapolate_mode`` is built."""
    if not isinstance(im, (np.ndarray, L.DeviceStack)):
        raise TypeError("wrong input image, should be np.ndarray")
    if extrapolate_mode != 'nearest':
        raise NotImplementedError(f"extrapolate_mode={extrapolate_mode!r}: only 'nearest' is built")
    return crop_neighboring_areas(im, [np.array(center, dtype=np.float64)[:3]], crop_sizes)[0]
