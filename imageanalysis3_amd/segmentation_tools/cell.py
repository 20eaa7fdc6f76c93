"""Bounding boxes of segmentation labels (reference: segmentation_tools/cell.py:598-611), from ONE device pass over the
label stack (``ia3_label_boxes_dev``) instead of one ``mask == cell_id`` and three reductions over the whole stack per
cell.  ``translate_segmentation`` (OpenCV) and the Cellpose drivers of that module stay the reference's.

All ``file:line`` citations are relative to the reference tree.
"""
import numpy as np

from .. import _lib as L
from ..classes.partition_spots import _device_form, _Resident

MAX_LABEL = 65535   # labels are carried as uint16


def _label_table(labels):
    """((65536, 7) int32 table [count, z0, z1, x0, x1, y0, y1] per label, image shape) of an integer / bool ndarray or a
    resident uint16 stack.  Negative labels cannot be carried (they would count as part of a mask)."""
    form, _ = _device_form(labels, vote=False)
    if np.dtype(form.dtype) != np.uint16:
        raise TypeError("a label image is an integer or bool array, got %s" % form.dtype)
    with _Resident(form) as stack:
        return L.label_boxes(stack, MAX_LABEL), tuple(int(n) for n in stack.shape)


def _grow(boxes, extend_pixel, shape):
    """(n, 3, 2) [start, stop) boxes grown by ``extend_pixel`` and clipped to the image (cell.py:608-609)."""
    e = int(extend_pixel)
    out = np.array(boxes, dtype=np.int64).reshape(-1, 3, 2)
    out[:, :, 0] = np.maximum(out[:, :, 0] - e, 0)
    out[:, :, 1] = np.minimum(out[:, :, 1] + e, np.array(shape)[None, :])
    return out.astype(np.int32)


def segmentation_label_boxes(labels, extend_pixel=1):
    """Every label of ``labels`` (ndarray or resident uint16 ``DeviceStack``) at once: ``(ids, boxes, counts)`` — the
    labels > 0 that occur in ascending order (int32), their (n, 3, 2) [start, stop) boxes grown by ``extend_pixel`` and
    clipped to the image (what ``segmentation_mask_2_bounding_box(labels, id, extend_pixel).array`` gives for each), and
    their voxel counts."""
    table, shape = _label_table(labels)
    ids = np.nonzero(table[:, 0] > 0)[0].astype(np.int32)
    return ids, _grow(table[ids, 1:].reshape(-1, 3, 2), extend_pixel, shape), table[ids, 0].copy()


def segmentation_mask_2_bounding_box(mask, cell_id=None, extend_pixel=1):
    """segmentation_tools/cell.py:598-611 — ``ImageCrop_3d`` around the voxels of ``cell_id`` where that label occurs,
    else around every non-zero voxel of ``mask``, grown by ``extend_pixel`` and clipped.  ``mask``: bool / integer
    ndarray or resident uint16 ``DeviceStack``."""
    from ..classes.preprocess import ImageCrop_3d
    table, shape = _label_table(mask)
    row = None
    if cell_id is not None:
        if cell_id == 0:
            raise NotImplementedError("the box of the background (cell_id 0) is not built")
        if 0 < cell_id <= MAX_LABEL and int(cell_id) == cell_id and table[int(cell_id), 0] > 0:
            row = table[int(cell_id), 1:]
    if row is None:
        hit = table[table[:, 0] > 0, 1:]
        if len(hit) == 0:   # np.min of no indices (cell.py:608)
            raise ValueError("zero-size array to reduction operation minimum which has no identity")
        row = np.stack([hit[:, 0::2].min(axis=0), hit[:, 1::2].max(axis=0)], axis=1).reshape(-1)
    return ImageCrop_3d(_grow(row, extend_pixel, shape)[0], shape)
