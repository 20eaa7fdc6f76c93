"""The label lookups of the reference's ``classes/partition_spots.py`` — same names, signatures and return types,
computed by the kernels of labels.hip (no CPU fallback): ``find_coordinate_intensities`` (:212-236) and the two static
methods of ``Spots_Partition`` that every caller of a spot table runs next, ``spots_to_labels`` (:113-140) and
``spots_to_DAPI`` (:143-157).  The pandas / CSV part of ``Spots_Partition`` (``run``, ``read_gene_list``,
``Merge_GeneCounts``, the batch functions) is host plumbing around these and stays the reference's.

All ``file:line`` citations are relative to the reference tree.

Images may be ndarrays or resident ``DeviceStack``s.  The device carries uint16 and float32 stacks: a bool or integer
ndarray travels as uint16 and the result is cast back to its dtype.  ``spots`` is a ``Spots3D`` or any (N, >= 4) table
whose columns 1..3 are z, x, y.  Rows with NaN coordinates are outside the contract (the reference's cast of NaN to
int32 is undefined).
"""
import numpy as np

from .. import _lib as L


def _coords(spots):
    """(n, 3) float64 z, x, y of a spot table (``Spots3D.to_coords()`` where there is one, else columns 1..3)."""
    if np.size(spots) == 0:
        return np.zeros((0, 3), dtype=np.float64)
    if hasattr(spots, "to_coords"):
        c = np.asarray(spots.to_coords())
    else:
        c = np.asarray(spots)
        if c.ndim != 2 or c.shape[1] < 4:
            raise IndexError("spots should be an (N, >= 4) table with z, x, y in columns 1..3, got shape %s" % (c.shape,))
        c = c[:, 1:4]
    if c.size == 0:
        return np.zeros((0, 3), dtype=np.float64)
    return np.ascontiguousarray(c, dtype=np.float64)


def _check_radius(search_radius):
    r = int(search_radius)
    if r != search_radius or r < 0:
        raise ValueError("search_radius should be a non-negative integer, got %r" % (search_radius,))
    if r > L.CUBE_MAX_RADIUS:
        raise NotImplementedError("search_radius %d: cubes of radius 0 to %d are built" % (r, L.CUBE_MAX_RADIUS))
    return r


def _device_form(image, vote):
    """What travels to the device for ``image`` and the dtype its values come back in: (DeviceStack or uint16 / float32
    ndarray, dtype or None).  ``vote``: a label image, where negative values are background; otherwise an integer value
    outside 0..65535 cannot be carried."""
    if isinstance(image, L.DeviceStack):
        if vote and image.dtype != np.uint16:
            raise TypeError("a resident label stack is uint16, got %s" % image.dtype)
        return image, None
    a = np.asarray(image)
    if a.ndim != 3:
        raise IndexError("a 3-D (z,x,y) stack is required, got ndim=%d" % a.ndim)
    if a.dtype == np.uint16 or (a.dtype == np.float32 and not vote):
        return a, None
    if a.dtype.kind == 'b':
        return a.astype(np.uint16), a.dtype
    if a.dtype.kind in 'iu':
        if a.size:
            lo, hi = int(a.min()), int(a.max())
            if hi > 65535 or (lo < 0 and not vote):
                raise NotImplementedError("integer images are carried as uint16: values %d..%d do not fit" % (lo, hi))
            if lo < 0:
                a = np.maximum(a, 0)   # the vote counts labels > 0 only
        return a.astype(np.uint16), np.asarray(image).dtype
    if vote:
        raise NotImplementedError("a label image is an integer or bool array, got %s" % a.dtype)
    raise TypeError("imageanalysis3_amd kernels take uint16 or float32 stacks, got %s" % a.dtype)


class _Resident(object):
    """``with _Resident(form) as stack``: the stack itself, or an upload that is freed on the way out."""

    def __init__(self, form):
        self._own = not isinstance(form, L.DeviceStack)
        self._stack = L.DeviceStack.upload(form) if self._own else form

    def __enter__(self):
        return self._stack

    def __exit__(self, *a):
        if self._own:
            self._stack.free()


def _form_dtype(form, back):
    return np.dtype(back) if back is not None else np.dtype(form.dtype)


def find_coordinate_intensities(image, spots, search_radius=5):
    """classes/partition_spots.py:212-236 — the (N, (2 search_radius + 1)^3) values around every spot: centre rounded
    half to even, offsets in C order of (dz, dx, dy), indices clamped into the image.  Image dtype."""
    r = _check_radius(search_radius)
    form, back = _device_form(image, vote=False)
    c = _coords(spots)
    if len(c) == 0:
        return np.zeros((0, (2 * r + 1) ** 3), dtype=_form_dtype(form, back))
    with _Resident(form) as stack:
        out = L.cube_gather(stack, c, r)
    return out if back is None else out.astype(back)


class Spots_Partition():
    """Only the two static lookups are part of this package; the class around them (DataFrames, CSV files) is the
    reference's ``classes/partition_spots.py``."""

    def __init__(self, *args, **kwargs):
        raise NotImplementedError("Spots_Partition(...) is the reference's pandas / CSV plumbing "
                                  "(ImageAnalysis3 classes/partition_spots.py); this package provides its static "
                                  "methods spots_to_labels and spots_to_DAPI")

    @staticmethod
    def spots_to_labels(segmentation_masks, spots, search_radius=10, verbose=True):
        """classes/partition_spots.py:113-140 — per spot the most frequent label > 0 in the cube around it (the smallest
        of equally frequent ones), -1 where the cube holds none.  int32.  Negative labels count as background."""
        if verbose:
            print(f"-- partition barcodes for {len(spots)} spots")
        r = _check_radius(search_radius)
        form, _ = _device_form(segmentation_masks, vote=True)
        c = _coords(spots)
        if len(c) == 0:
            return np.zeros(0, dtype=np.int32)
        with _Resident(form) as stack:
            return L.cube_labels(stack, c, r)

    @staticmethod
    def spots_to_DAPI(dapi_im, spots, search_radius=5, verbose=True):
        """classes/partition_spots.py:143-157 — per spot the largest value in the cube around it, image dtype."""
        if verbose:
            print(f"-- calculate local DAPI signal for {len(spots)} spots")
        r = _check_radius(search_radius)
        form, back = _device_form(dapi_im, vote=False)
        c = _coords(spots)
        if len(c) == 0:
            return np.zeros(0, dtype=_form_dtype(form, back))
        with _Resident(form) as stack:
            out = L.cube_max(stack, c, r)
        return out if back is None else out.astype(back)
