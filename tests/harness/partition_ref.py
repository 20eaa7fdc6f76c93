"""NumPy statement of what labels.hip computes: bounding boxes and counts of a label image, and the clamped cubes around
spot centres with their vote, contains test, maximum and gather (reference: segmentation_tools/cell.py:598-611,
classes/partition_spots.py:113-157, 212-236).

Written from the description of the operations; tests/test_partition_cpu.py holds it to the reference's
own outputs (tests/golden/partition.npz) exactly.  The GPU machine has no reference: device tests on other inputs compare
with this file.
"""
import numpy as np


def boxes(labels, max_label=None):
    """(max_label + 1, 7) int32 rows [count, z0, z1, x0, x1, y0, y1]: voxel count and tight [start, stop) bounds per
    label, zeros for a label that does not occur and for row 0."""
    lab = np.asarray(labels)
    top = int(lab.max()) if max_label is None else int(max_label)
    out = np.zeros((top + 1, 7), dtype=np.int32)
    counts = np.bincount(lab[(lab > 0) & (lab <= top)].ravel().astype(np.int64), minlength=top + 1)
    for l in np.nonzero(counts)[0]:
        hit = np.nonzero(lab == l)
        out[l] = [counts[l]] + [v for ix in hit for v in (ix.min(), ix.max() + 1)]
    return out


def offsets(radius):
    """((2 radius + 1)^3, 3) offsets (dz, dx, dy) in C order: dz slowest, dy fastest."""
    r = np.arange(-radius, radius + 1)
    return np.stack(np.meshgrid(r, r, r, indexing="ij"), axis=-1).reshape(-1, 3)


def cube_indices(shape, centres_zxy, radius):
    """(n, (2 radius + 1)^3, 3) voxel indices: centre rounded half to even, plus every offset, clamped into the image."""
    c = np.round(np.asarray(centres_zxy, dtype=np.float64)).astype(np.int64).reshape(-1, 3)
    idx = c[:, None, :] + offsets(radius)[None, :, :]
    return np.clip(idx, 0, np.array(shape) - 1)


def gather(image, centres_zxy, radius):
    im = np.asarray(image)
    idx = cube_indices(im.shape, centres_zxy, radius)
    return im[idx[..., 0], idx[..., 1], idx[..., 2]]


def vote(labels, centres_zxy, radius):
    """Most frequent label > 0 per cube, the smallest of equally frequent ones, -1 for none (int32)."""
    out = []
    for cube in gather(labels, centres_zxy, radius):
        vals, counts = np.unique(cube[cube > 0], return_counts=True)
        out.append(vals[np.argmax(counts)] if len(vals) else -1)
    return np.array(out, dtype=np.int32)


def contains(labels, centres_zxy, radius, target):
    cubes = gather(labels, centres_zxy, radius)
    hit = (cubes == np.asarray(target).reshape(-1, 1)).any(axis=1)
    return np.where(hit, 1, -1).astype(np.int32)


def cube_max(image, centres_zxy, radius):
    cubes = gather(image, centres_zxy, radius)
    return np.max(cubes, axis=1) if len(cubes) else np.zeros(0, dtype=np.asarray(image).dtype)
