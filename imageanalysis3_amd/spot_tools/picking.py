"""spot_tools/picking.py — of the reference's module only ``assign_spots_to_chromosomes`` (:767-794), which
``segmentation_tools.chromosome.select_candidate_chromosomes`` is built on: the nearest chromosome of every spot, found on
the device (``ia3_assign_nearest_dev``) with SciPy's ``cdist`` arithmetic and ``np.argmin``'s tie and NaN
rules, bit for bit.  The rest of the module (naive / EM picking, scoring, the distance maps) stays the reference's.

All ``file:line`` citations are relative to the reference tree.
"""
import numpy as np

from .. import _lib as L
from . import _distance_zxy


def assign_spots_to_chromosomes(spots, chrom_coords, distance_zxy=_distance_zxy, dist_norm=2):
    """picking.py:767-794 — list with, per row of ``chrom_coords`` (z, x, y pixels), the rows of ``np.array(spots)``
    (intensity, z, x, y, ...) that are nearer to it than to any other chromosome, in ascending row order; the first of
    equally near chromosomes takes the spot.  ``[[] for each chromosome]`` when there is no spot.  ``distance_zxy``: pixel
    size in nm along z, x, y.  ``dist_norm`` has no effect, as in the reference (``cdist`` is called without it)."""
    _chrom_zxys = np.array(chrom_coords) * np.array(distance_zxy)
    _spots = np.array(spots)
    if len(_spots) == 0:
        return [[] for _i, _chrom_zxy in enumerate(_chrom_zxys)]
    _zxys = _spots[:, 1:4] * np.array(distance_zxy)
    from ..segmentation_tools.chromosome import _cdist_table
    _zxys, _chrom_zxys = _cdist_table(_zxys, "XA"), _cdist_table(_chrom_zxys, "XB")
    if len(_chrom_zxys) == 0:
        raise ValueError("attempt to get argmin of an empty sequence")
    _assign_flags = L.assign_nearest(_zxys, _chrom_zxys)
    return split_rows_by_owner(_spots, _assign_flags, len(_chrom_zxys))


def split_rows_by_owner(_spots, owner, n_owners):
    """``[_spots[np.where(owner == i)] for i in range(n_owners)]`` (:792) from one stable sort of ``owner``."""
    order = np.argsort(owner, kind="stable")
    bounds = np.searchsorted(owner[order], np.arange(n_owners + 1))
    return [_spots[order[a:b]] for a, b in zip(bounds[:-1], bounds[1:])]
