"""TEST HARNESS — inputs of the label-lookup fixtures (tests/golden/partition.npz): label images and intensity stacks
that scripts/make_partition_golden.py and the tests build alike, and the spot coordinates the fixture was made at.
Only coordinates, radii and the reference's outputs are stored in the fixture."""
import itertools

import numpy as np

FCI_RADII = (0, 1, 3)          # find_coordinate_intensities
VOTE_RADII = (0, 3, 4, 10)     # spots_to_labels
DAPI_RADII = (0, 5)            # spots_to_DAPI
DAPI_SHAPE = (9, 40, 50)
SEG_SHAPE = (20, 300, 260)


def small_labels():
    """(5, 37, 67): rows are no multiple of 64.  A label that changes inside a wavefront (2), one whose run crosses a
    wavefront and a row (300), a one-voxel label (17), one in two pieces (40), label 65535, gaps in the ids, and two
    labels (9 first in memory, then 5) that tie in a cube centred on the background column between them."""
    lab = np.zeros((5, 37, 67), np.int32)
    lab[1:4, 12:19, 20:60] = 1000
    lab[0, 0, 3:41] = 2
    lab.reshape(-1)[50:88] = 300
    lab[2, 20, 33] = 17
    lab[1, 5:8, 5:9] = 40
    lab[4, 30:36, 60:67] = 40
    lab[3, 10:14, 0:5] = 65535
    lab[:, 20:30, 10:12] = 9
    lab[:, 20:30, 13:15] = 5
    return lab


def distinct_labels():
    """(3, 64, 128): every voxel has a label of its own, 1..24576 in memory order."""
    return np.arange(1, 3 * 64 * 128 + 1, dtype=np.int32).reshape(3, 64, 128)


def one_label():
    return np.full((1, 1, 1), 7, np.int32)


def label_cases():
    from conftest import seg_labels
    return {"seg": seg_labels(SEG_SHAPE), "small": small_labels(), "distinct": distinct_labels(), "one": one_label()}


SPECIAL = {   # name -> {what: (z, x, y)}
    "seg": {"background": (10., 160., 20.)},
    "small": {"background": (2., 33., 30.), "tie": (2., 25., 12.)},
    "distinct": {},
    "one": {},
}


def spot_coords(name, shape):
    """(n, 3) float64 centres: halves (rounded to the even neighbour), the eight corners, centres outside the image (the
    cube collapses onto a face, an edge or a corner), the case's special spots, and a dozen scattered ones."""
    Z, X, Y = shape
    pts = [(2.5, 3.5, 4.5), (0.5, 1.5, 2.5), (-0.5, 0.5, 1.5), (Z - 1.5, X - 0.5, Y - 2.5)]
    pts += list(itertools.product((0., Z - 1.), (0., X - 1.), (0., Y - 1.)))
    pts += [(-3., -7., -2.), (Z + 4., X + 9., Y + 5.), (Z / 2., -20., Y + 30.), (-100.2, 1e4, 5.), (Z / 2., X / 2., -1e6)]
    pts += [SPECIAL[name][k] for k in sorted(SPECIAL[name])]
    rng = np.random.RandomState(len(name) + Z + X + Y)
    pts += [tuple(v) for v in rng.uniform(-2., np.array(shape) + 2., size=(12, 3))]
    return np.array(pts, dtype=np.float64)


def special_index(name, what, shape):
    """Row of ``spot_coords(name, shape)`` that holds the special spot ``what``."""
    c = spot_coords(name, shape)
    return int(np.nonzero((c == np.array(SPECIAL[name][what])).all(axis=1))[0][0])


def spot_table(coords, dtype=np.float64):
    """(n, 11) spot table with the centres in columns 1..3."""
    t = np.zeros((len(coords), 11), dtype=dtype)
    t[:, 1:4] = coords
    return t


def dapi_u16():
    return np.random.RandomState(7).randint(0, 60000, size=DAPI_SHAPE).astype(np.uint16)


def dapi_f32(nan=False):
    """float32 stack with negative values; ``nan``: with NaNs planted at a corner and in the middle."""
    im = np.random.RandomState(8).normal(100., 400., size=DAPI_SHAPE).astype(np.float32)
    if nan:
        im[0, 0, 0] = np.nan
        im[4, 20, 25] = np.nan
    return im
