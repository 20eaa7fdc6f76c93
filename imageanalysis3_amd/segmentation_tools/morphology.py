"""3-D binary morphology, hole filling and connected-component labelling on the device (csrc/morph.hip):
the ``scipy.ndimage`` / ``skimage.morphology`` operators that ``segmentation_tools/chromosome.py`` of the reference is
made of, bit for bit.

Every function takes a bool / integer ndarray or a resident ``DeviceStack`` (a uint16 mask, 0 / non-zero) and answers in
the form it was given: an ndarray of the input's dtype, or a new resident stack.  Structuring elements are
``ball(r)``, r = 0..2 (``ball(1)`` is SciPy's default 6-neighbour cross); labelling is 6-connected.

All ``file:line`` citations are relative to the reference tree.
"""
import numpy as np

from .. import _lib as L

__all__ = ["ball", "binary_erosion", "binary_dilation", "binary_closing", "binary_fill_holes", "label",
           "remove_small_objects", "label_centers"]


def ball(radius, dtype=np.uint8):
    """``skimage.morphology.ball(radius)``: the (2 r + 1)^3 array that is 1 where dz^2 + dx^2 + dy^2 <= r^2."""
    r = int(radius)
    g = np.arange(-r, r + 1)
    z, x, y = np.meshgrid(g, g, g, indexing="ij")
    return (z * z + x * x + y * y <= r * r).astype(dtype)


def _radius(structure):
    """The r of a structuring element given as ``None`` (SciPy's default cross, ball(1)), an int, or ``ball(r)`` itself."""
    if structure is None:
        return 1
    if np.ndim(structure) == 0:
        r = int(structure)
    else:
        s = np.asarray(structure)
        r = (s.shape[0] - 1) // 2 if s.ndim == 3 and len(set(s.shape)) == 1 and s.shape[0] % 2 == 1 else -1
        if r < 0 or not np.array_equal(s != 0, ball(r) != 0):
            raise NotImplementedError("the device operators take ball(r) as the structuring element (r = 0..%d; 18- and "
                                      "26-connected elements are not built)" % L.MORPH_MAX_RADIUS)
    if r < 0 or r > L.MORPH_MAX_RADIUS:
        raise NotImplementedError("ball(%d): the bit-row operators are built for r = 0..%d" % (r, L.MORPH_MAX_RADIUS))
    return r


class _Mask(object):
    """``with _Mask(image) as stack``: the resident uint16 mask of ``image`` (uploaded and freed here unless it already is
    a ``DeviceStack``); ``back(result_stack)`` gives the result in the caller's form."""

    def __init__(self, image):
        self._own = not isinstance(image, L.DeviceStack)
        if self._own:
            a = np.asarray(image)
            if a.ndim != 3:
                raise IndexError("a 3-D (z,x,y) mask is required, got ndim=%d" % a.ndim)
            if a.dtype.kind not in "biu":
                raise TypeError("a mask is a bool or integer array, got %s" % a.dtype)
            self.dtype = a.dtype
            self._host = np.ascontiguousarray(a != 0, dtype=np.uint16)
        else:
            if np.dtype(image.dtype) != np.uint16:
                raise TypeError("a resident mask is a uint16 stack, got %s" % image.dtype)
            self._stack = image

    def __enter__(self):
        if self._own:
            self._stack = L.DeviceStack.upload(self._host)
        return self

    @property
    def stack(self):
        return self._stack

    def back(self, out):
        if not self._own:
            return out
        try:
            return out.download().astype(self.dtype)
        finally:
            out.free()

    def __exit__(self, *a):
        if self._own:
            self._stack.free()


def _morph(image, op, structure, border):
    r = _radius(structure)
    with _Mask(image) as m:
        return m.back(L.binary_morph(m.stack, op, r, border))


def binary_erosion(image, structure=None, border_value=0):
    """``scipy.ndimage.binary_erosion(image, structure, border_value=border_value)`` (one iteration, no mask)."""
    return _morph(image, L.MORPH_ERODE, structure, border_value)


def binary_dilation(image, structure=None, border_value=0):
    """``scipy.ndimage.binary_dilation(image, structure, border_value=border_value)`` (one iteration, no mask)."""
    return _morph(image, L.MORPH_DILATE, structure, border_value)


def binary_closing(image, structure=None):
    """``skimage.morphology.closing`` of a mask: dilation, then an erosion for which the outside of the volume counts as
    set (the morphological-closing convention; ``scipy.ndimage.binary_closing`` erodes with the outside clear instead)."""
    return _morph(image, L.MORPH_CLOSE, structure, 0)


def binary_fill_holes(image, structure=None):
    """``scipy.ndimage.binary_fill_holes(image, structure)`` for the 6-neighbour cross (``None`` or ``ball(1)``): a hole is
    a 6-connected component of the background that touches no face of the volume."""
    if _radius(structure) != 1:
        raise NotImplementedError("holes are filled for the 6-neighbour cross (ball(1)) only: with a larger element hole "
                                  "filling is no longer plain connectivity")
    with _Mask(image) as m:
        return m.back(L.binary_fill_holes(m.stack))


def label(image):
    """``scipy.ndimage.label(image)`` with the default structure: ``(labels, n)``, labels int32, the 6-connected components
    numbered 1..n in raster order of their first voxel.  An ndarray gives an ndarray, a resident mask ``DeviceLabels``."""
    with _Mask(image) as m:
        lab = L.label(m.stack)
        if isinstance(image, L.DeviceStack):
            return lab, lab.n
        try:
            return lab.download(), lab.n
        finally:
            lab.free()


class _Labels(object):
    """``with _Labels(labels) as dev``: a ``DeviceLabels`` / resident uint16 stack for an integer ndarray (freed here) or
    the resident object itself."""

    def __init__(self, labels):
        self._own = not isinstance(labels, (L.DeviceLabels, L.DeviceStack))
        self._in = labels
        if self._own:
            a = np.asarray(labels)
            if a.ndim != 3:
                raise IndexError("a 3-D (z,x,y) label volume is required, got ndim=%d" % a.ndim)
            if a.dtype.kind not in "iu":
                raise TypeError("labels are an integer array, got %s" % a.dtype)
            if a.size and (int(a.min()) < 0 or int(a.max()) > 2 ** 31 - 1):
                raise NotImplementedError("labels 0 .. 2^31 - 1 are carried (int32)")
            self.dtype = a.dtype
            self._host = a

    def __enter__(self):
        self.dev = L.DeviceLabels.upload(self._host) if self._own else self._in
        return self

    def __exit__(self, *a):
        if self._own:
            self.dev.free()


def _max_label(dev, max_label):
    if max_label is not None:
        return int(max_label)
    return dev.n if isinstance(dev, L.DeviceLabels) else L.MAX_LABELS16


def remove_small_objects(ar, min_size=64, max_label=None):
    """``skimage.morphology.remove_small_objects(ar, min_size)``: on a labelled array, labels with fewer than ``min_size``
    voxels become 0 and the others keep their numbers; a bool array is labelled first (6-connected) and comes back bool.
    ``max_label``: the largest label of a resident volume when the caller knows it (``DeviceLabels`` carry theirs)."""
    if not isinstance(ar, (L.DeviceLabels, L.DeviceStack)) and np.asarray(ar).dtype.kind == "b":
        with _Mask(ar) as m:
            with L.label(m.stack) as lab, L.remove_small_labels(lab, lab.n, min_size) as kept:
                return kept.download() != 0
    with _Labels(ar) as h:
        out = L.remove_small_labels(h.dev, _max_label(h.dev, max_label), min_size)
        if not h._own:
            return out
        try:
            return out.download().astype(h.dtype)
        finally:
            out.free()


def label_centers(labels, max_label=None):
    """For the labels 1..max_label (default: the largest label) of an integer ndarray, ``DeviceLabels`` or resident uint16
    label stack: ``(centers, counts)`` — (max_label, 3) float64, what ``_calculate_binary_center(labels == l)``
    (segmentation_tools/chromosome.py:4-10) gives per label (per axis the mean of the indices > 0; NaN where a label has
    none), and the (max_label,) int64 voxel counts (0 for a label that does not occur)."""
    with _Labels(labels) as h:
        return L.label_centers(h.dev, _max_label(h.dev, max_label))
