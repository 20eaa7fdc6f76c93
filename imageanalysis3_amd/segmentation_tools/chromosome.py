"""Candidate chromosomes of a whole (Z, X, Y) stack on the device (reference: segmentation_tools/chromosome.py:264-361
``find_candidate_chromosomes``, which ``Field_of_View._find_candidate_chromosomes_by_segmentation`` calls at
classes/field_of_view.py:2127): plane medians, range filter, percentile threshold, opening, hole filling, closing,
labelling, size filter and centres in one library call (``ia3_find_candidate_chromosomes_dev``), bit for
bit.  The operators themselves are ``segmentation_tools.morphology``.

All ``file:line`` citations are relative to the reference tree.
"""
import time

import numpy as np

from .. import _lib as L

_COMPOSE = ("compose it from segmentation_tools.morphology (ball, binary_erosion, binary_dilation, binary_closing, "
            "binary_fill_holes, label, remove_small_objects, label_centers)")


def _image_form(_chrom_im):
    """What goes to the device for ``_chrom_im``: the resident stack or chromosome image itself, or a uint16 / float32
    ndarray."""
    if isinstance(_chrom_im, (L.DeviceStack, L.ChromImage)):
        return _chrom_im
    a = np.asarray(_chrom_im)
    if a.ndim != 3:
        raise IndexError("a 3-D (z,x,y) stack is required, got ndim=%d" % a.ndim)
    if a.dtype == np.float64:
        b = a.astype(np.float32)
        if not np.array_equal(b.astype(np.float64), a):
            raise NotImplementedError(
                "float64 stacks are not built: a float64 image is taken only when every value is exact in float32 (it is "
                "then processed as that float32 image); this one is not")
        a = b
    return L.as_stack_array(a)


def _check_medians(a):
    """chromosome.py:296 divides every plane by its median: 0 or a non-finite value is outside the contract."""
    for z, lyr in enumerate(a):
        m = np.median(lyr)
        if m == 0 or not np.isfinite(m):
            raise ValueError("plane %d has the median %s: the layer adjustment divides by it" % (z, m))


def find_candidate_chromosomes(_chrom_im,
                               _adjust_layers=False,
                               _filt_size=3,
                               _binary_per_th=99.5,
                               _morphology_size=1,
                               _min_label_size=100,
                               _random_walk_beta=10,
                               _num_threads=12,
                               _verbose=True,
                               _return_label=False):
    """segmentation_tools/chromosome.py:264-361 — centres (z, x, y pixels, (n, 3) float64, ``np.array([])`` when there is
    no object) of the candidate chromosomes of ``_chrom_im``: a uint16 / float32 ndarray or a resident ``DeviceStack``
    (never downloaded); a float64 ndarray only when every value is exact in float32.  A resident ``ChromImage`` (what
    ``classes.field_of_view.generate_chrom_im`` returns with ``return_device=True``, or ``ChromImage.upload`` of a
    float64 ndarray) is processed in float64, as the reference processes a float64 image: float64 plane medians, quotients
    and seed.

    ``_adjust_layers``, ``_random_walk_beta`` and ``_num_threads`` have no effect: the reference ignores the first, its
    random walker returns the labels it was given (none of them is 0, :326), and no process pool is started here.
    ``_filt_size`` 1..5 and ``_morphology_size`` 1 are built, at most 65535 components (NotImplementedError otherwise).
    ``_return_label=True``: ``(coords, kept_label)`` with the uint16 label stack of :337 as a resident ``DeviceStack``."""
    lo, hi = L.CHROM_FILT_SIZES
    if int(_filt_size) != _filt_size or not lo <= int(_filt_size) <= hi:
        raise NotImplementedError("_filt_size %s: the range filter is built for sizes %d to %d" % (_filt_size, lo, hi))
    if int(_morphology_size) != _morphology_size or int(_morphology_size) != 1:
        raise NotImplementedError("_morphology_size %s: only ball(1) is built into the fused call (with a larger ball "
                                  "hole filling is no longer plain connectivity); %s" % (_morphology_size, _COMPOSE))
    form = _image_form(_chrom_im)
    own = not isinstance(form, (L.DeviceStack, L.ChromImage))
    if own:
        _check_medians(form)
    if _verbose:
        print(f"-- adjust seed image with filter size={_filt_size}")
        print(f"-- binarize image with threshold: {_binary_per_th}%")
        print(f"-- erosion and dialation with size={_morphology_size}.")
        print(f"-- find close objects.")
        print(f"-- random walk segmentation, beta={_random_walk_beta}.")
        print(f"-- find objects larger than size={_min_label_size}")
    stack = L.DeviceStack.upload(form) if own else form
    try:
        _start = time.time()
        coords, _, kept = L.find_candidate_chromosomes(stack, _filt_size, _binary_per_th, _morphology_size,
                                                       np.ceil(_min_label_size), return_label=_return_label)
    finally:
        if own:
            stack.free()
    if _verbose:
        print(f"-- {len(coords)} objects are found by segmentation.")
        print(f"- Start multiprocessing caluclate chromosome coordinates with {_num_threads} threads", end=' ')
        print(f"in {time.time()-_start:.3f}s.")
    _chrom_coords = coords if len(coords) else np.array([])
    return (_chrom_coords, kept) if _return_label else _chrom_coords


def _calculate_binary_center(_binary_label):
    """segmentation_tools/chromosome.py:4-10 — per axis the mean of the index over the set voxels whose index on that
    axis is > 0 (NaN when there is none): array of 3 float64.  ``_binary_label``: bool / 0-1 integer ndarray or a
    resident uint16 mask."""
    from .morphology import _Mask
    with _Mask(_binary_label) as m:
        if m._own:
            return L.label_centers(m.stack, 1)[0][0]
        with L.binary_morph(m.stack, L.MORPH_DILATE, 0) as one:   # 0 / non-zero -> 0 / 1
            return L.label_centers(one, 1)[0][0]


def find_candidate_chromosomes_in_nucleus(_chrom_im, _dna_im, _dna_mask=None,
                                          _chr_seed_size=200,
                                          _filt_size=3,
                                          _num_of_iter=10,
                                          _percent_th_3chr=97.5,
                                          _percent_th_2chr=85,
                                          _use_percent_chr_area=False,
                                          _fold_3chr=6,
                                          _fold_2chr=4,
                                          _std_ratio=3,
                                          _morphology_size=1,
                                          _min_label_size=30,
                                          _random_walk_beta=15,
                                          _num_threads=4,
                                          _verbose=True):
    """segmentation_tools/chromosome.py:51-259 — not built (Otsu, disk(10), regionprops, the size-split branches)."""
    raise NotImplementedError("find_candidate_chromosomes_in_nucleus is not built; " + _COMPOSE)


def select_candidate_chromosomes(_cand_chrom_coords,
                                 _spots_list,
                                 _cand_spot_intensity_th=0.5,
                                 _good_chr_loss_th=0.4,
                                 _verbose=True,
                                 ):
    """segmentation_tools/chromosome.py:363-406 — the candidates (z, x, y pixels) that lose a spot of intensity >=
    ``_cand_spot_intensity_th`` in at most ``_good_chr_loss_th`` of the rounds of ``_spots_list``, after the worst
    candidate has been removed one at a time and its spots handed to their next nearest candidate:
    ``np.array(kept rows).copy()``, the reference's array, from one library call (``ia3_select_chromosomes_dev``,
    DESIGN.md §21).  ``_good_chr_loss_th >= 1`` and an empty ``_spots_list`` return every candidate without the device;
    no candidate at all, or the removal of the last one, raises ``NoChromosomeLeft`` (a ``ValueError``, as ``max()`` of the
    reference's empty list)."""
    _cand_chrom_coords = list(_cand_chrom_coords)
    return _select_chromosomes(_cand_chrom_coords, _spots_list, _cand_spot_intensity_th, _good_chr_loss_th, _verbose)[0]


# two bases: the reference's max([]) raises ValueError; callers from before this was built expect NotImplementedError
class NoChromosomeLeft(ValueError, NotImplementedError):
    pass


_NONE_LEFT = ("max() arg is an empty sequence: no candidate chromosome is left for spot_tools.picking."
              "assign_spots_to_chromosomes to assign spots to")


def _cdist_table(zxy, name):
    """What ``cdist`` makes of an argument, with its errors: a 2-D float64 table; three columns here."""
    t = np.asarray(zxy, dtype=np.float64)
    if t.ndim != 2:
        raise ValueError("%s must be a 2-dimensional array." % name)
    if t.shape[1] != 3:
        raise ValueError("XA and XB must have the same number of columns (i.e. feature dimension.): z, x, y; %s has %d"
                         % (name, t.shape[1]))
    return t


def _pack_rounds(_spots_list, _cand_spot_intensity_th, distance_zxy):
    """:380-383 and picking.py:780-783 for every round: (selected rows per round, their scaled z, x, y of all rounds packed
    into one float64 table, the R + 1 row offsets of the rounds)."""
    sels, tables, starts = [], [], [0]
    for _spots in _spots_list:
        _spots = np.array(_spots)
        _sel_spots = _spots[_spots[:, 0] >= _cand_spot_intensity_th]
        sels.append(_sel_spots)
        if len(_sel_spots):
            tables.append(_cdist_table(_sel_spots[:, 1:4] * np.array(distance_zxy), "XA"))
        starts.append(starts[-1] + len(_sel_spots))
    zxys = np.concatenate(tables) if tables else np.zeros((0, 3), dtype=np.float64)
    return sels, zxys, np.array(starts, dtype=np.int32)


def _select_chromosomes(_cand_chrom_coords, _spots_list, _cand_spot_intensity_th, _good_chr_loss_th, _verbose,
                        owners=False):
    """The loop of :371-406 on the list ``_cand_chrom_coords``: (chrom_coords, info), info = dict of ``removed`` (original
    indices in removal order), ``kept`` (original indices of the rows of chrom_coords), ``lost`` (rounds without a spot per
    candidate, at its removal for a removed one; None when the loop never looked at a spot) and, with ``owners``, ``sels``
    (the selected rows of every round) and ``owner`` (per round the row of chrom_coords that owns each selected row)."""
    from .. import _distance_zxy
    n_cand = len(_cand_chrom_coords)
    if _verbose:
        print(f"- start select from {n_cand} chromosomes with loss threshold={_good_chr_loss_th}")
    if n_cand == 0:
        raise NoChromosomeLeft(_NONE_LEFT)
    info = dict(removed=np.zeros(0, dtype=np.int32), kept=np.arange(n_cand), lost=None)
    n_rounds = len(_spots_list)
    if 1 > _good_chr_loss_th and n_rounds > 0:      # :375-377: every flag starts at 1; np.mean of no rounds is NaN
        _chrom_zxys = _cdist_table(np.array(_cand_chrom_coords) * np.array(_distance_zxy), "XB")
        sels, zxys, starts = _pack_rounds(_spots_list, _cand_spot_intensity_th, _distance_zxy)
        res = L.select_chromosomes(zxys, starts, _chrom_zxys, _good_chr_loss_th, return_owner=owners)
        alive = np.ones(n_cand, dtype=bool)
        for c, lost in zip(res["removed"], res["removed_lost"]):
            if _verbose:
                print(f"-- remove chr id {int(alive[:c].sum())}, percentage of lost rounds:{np.float64(lost) / n_rounds:.3f}.")
            alive[c] = False
        if res["empty"]:
            raise NoChromosomeLeft(_NONE_LEFT)
        info = dict(removed=res["removed"], kept=np.flatnonzero(alive), lost=res["lost"])
        if owners:
            row = np.cumsum(alive) - 1             # original index -> row of chrom_coords
            info["sels"] = sels
            info["owner"] = [row[res["owner"][a:b]] for a, b in zip(starts[:-1], starts[1:])]
    _chrom_coords = np.array([_cand_chrom_coords[i] for i in info["kept"]]).copy()
    if _verbose:
        print(f"-- {len(_chrom_coords)} chromosomes are kept.")
    return _chrom_coords, info


def identify_chromosomes(chrom_im, dapi_im=None,
                         seed_gfilt_size=0.75, background_gfilt_size=7.5,
                         chrom_snr_th=1.5, dapi_snr_th=2,
                         morphology_size=1, min_label_size=25,
                         num_threads=12,
                         return_seed_im=False,
                         verbose=True):
    """segmentation_tools/chromosome.py:409- — not built (the reference's version uses ``np.float``)."""
    raise NotImplementedError("identify_chromosomes is not built; " + _COMPOSE)
