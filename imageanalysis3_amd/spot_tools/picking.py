"""spot_tools/picking.py — of the reference's module ``assign_spots_to_chromosomes`` (:767-794), which
``segmentation_tools.chromosome.select_candidate_chromosomes`` is built on, and the population picker (:1567-2342):
``convert_spots_to_hzxys``, ``extract_intensities``, ``pick_spots_by_intensities``, ``chromosome_center_dists``,
``local_center_dists``, ``generate_reference_from_population`` (E-step), ``cum_val``, ``slow_cum_val``,
``pick_spots_by_scores`` (M-step) and ``evaluate_differences``, run on the device by csrc/pick.hip on a
population that is uploaded once (``upload_population`` / ``_lib.PickPopulation``) and stays resident.  Every result is the
reference's bit for bit on the same host: distances in NumPy's two norm forms, ``np.nanmean`` in row order, the literal
``cum_val`` search, ``np.argmax`` / ``np.nanmax`` selection, and scores from this host's ``np.log`` (tabled per search
node).  ``em_pick_spots`` is the loop the reference's users write around these; it is not a reference name.

The per-cell pickers (csrc/cellpick.hip): ``merge_spot_list`` (:662), ``naive_pick_spots`` (:14),
``naive_pick_spots_for_chromosomes`` (:797), ``dynamic_pick_spots_for_chromosomes`` (:902) and
``EM_pick_spots_for_chromosomes`` (:1204) with the reference's arguments, returns, messages and quirks, each the one-cell
case of a flat form on a resident population of cells (``_lib.CellPickPopulation``; not reference names):
``population_merge_spot_lists``, ``population_naive_pick_spots``, ``population_dynamic_pick_spots`` and
``population_EM_pick_spots`` take a list of cells ``(cell_cand_spots, region_ids, chrom_coords)`` and return per cell what
the reference's function returns for it.  The candidates go up once, the merged lists are made and kept on the device, the
forward pass of the dynamic program runs one workgroup per cell, and per EM iteration per-spot scores go up and dynamic
scores and pointers come back; the E-step's references and scores come from a ``_lib.ScorePopulation`` of every
(cell, chromosome), ``np.log`` is this host's.  The backward pass and the reference's bookkeeping are host Python.
``_optimized_score_combinations`` and ``_all_score_combinations`` (:1531, :1552) are host functions.

THE TIE RULE.  The reference sorts with ``np.argsort``'s default kind, which is not stable: on equal keys its order, and
with it the reference's own output, depends on the host's CPU.  Here equal keys are taken by ascending index, NaN last
(``kind='stable'``); the fixture is the reference run with its argsort pinned to that order.

LIMITS, each NotImplementedError: at most ``_lib.IA3_CELLPICK_MAX_CHROM`` (6) chromosomes per cell, refused before anything
is uploaded, and ``_lib.IA3_CELLPICK_MAX_SPOTS`` (64) merged spots per region, which only the merge can count: the merge
kernel runs first, and the refusal comes after it and before the E-step and the forward pass.  A spot of the next region
walks at most ``_lib.IA3_CELLPICK_MAX_TUPLES`` index tuples (more arise only when every score of a chromosome is infinite);
beyond that the forward pass leaves the spot and the call raises.  Also not built: ``make_plot=True``, a ``dist_norm`` other
than 2, a 'cdf' ``score_metric`` with other than 'cdf' references (and the reverse), and the legacy single-chromosome
``dynamic_pick_spots`` (:306), ``EM_pick_spots`` (:389), ``old_spot_score_in_chromosome``, ``distance_score_in_chromosome``,
``generate_distance_score_pool``, ``generate_spot_score_pool`` and
``screen_RNA_based_on_refs``.

All ``file:line`` citations are relative to the reference tree.
"""
import bisect
import itertools
import time

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


# ---- the population picker (:1567-2342) ---------------------------------------------------------------------------------

def convert_spots_to_hzxys(spot_list, pix_size=_distance_zxy, normalize_spot_background=False):
    """picking.py:2318-2342 — per entry of ``spot_list`` the columns (h, z, x, y) with z, x, y scaled to nm (``[]`` for an
    empty entry, a 1-D row for a 1-D spot); ``normalize_spot_background`` divides h by the column after the coordinates.
    Host NumPy, as in the reference: it prepares the ragged lists that ``upload_population`` packs."""
    _hzxys_list = []
    pix_size = np.array(pix_size)
    _nd = 1 + len(pix_size)
    for _spots in spot_list:
        if len(_spots) == 0:
            _hzxys_list.append([])
            continue
        _spots = np.array(_spots).copy()
        if _spots.ndim == 1:
            _hzxy = _spots[:_nd]
            _hzxy[1:_nd] = _hzxy[1:_nd] * pix_size
            if normalize_spot_background:
                _hzxy[0] = _hzxy[0] / _spots[_nd]
            _hzxys_list.append(_hzxy)
        elif _spots.ndim == 2:
            _hzxys = _spots[:, :_nd]
            _hzxys[:, 1:_nd] = _hzxys[:, 1:_nd] * pix_size
            if normalize_spot_background:
                _hzxys[:, 0] = _hzxys[:, 0] / _spots[:, _nd]
            _hzxys_list.append(_hzxys)
        else:
            raise IndexError("_spots should be 1d or 2d array.")
    return _hzxys_list


def extract_intensities(cand_hzxys):
    """picking.py:1567-1576 — per region ``[]``, the h of a 1-D row, or the h column of a table."""
    _ints = []
    for _hzxys in cand_hzxys:
        if len(_hzxys) == 0:
            _ints.append([])
        elif np.ndim(np.array(_hzxys)) == 1:
            _ints.append(_hzxys[0])
        elif np.ndim(np.array(_hzxys)) == 2:
            _ints.append(_hzxys[:, 0])
    return _ints


def _pack(cand_hzxys_list):
    """(n, 4) table, P*R + 1 offsets and P*R 1-D flags of ragged ``cand_hzxys_list[p][r]``."""
    P = len(cand_hzxys_list)
    R = len(cand_hzxys_list[0])
    parts, counts, flags = [], [], []
    for _regions in cand_hzxys_list:
        if len(_regions) != R:
            raise IndexError("every chromosome should have %d regions, one has %d" % (R, len(_regions)))
        for _e in _regions:
            if len(_e) == 0:
                counts.append(0)
                flags.append(0)
                continue
            _t = np.array(_e, dtype=np.float64)
            if _t.ndim not in (1, 2) or _t.shape[-1] != 4:
                raise IndexError("Wrong input shape for cand_hzxys:_hzxys")
            flags.append(1 if _t.ndim == 1 else 0)
            _t = _t.reshape(-1, 4)
            parts.append(_t)
            counts.append(len(_t))
    table = np.concatenate(parts) if parts else np.zeros((0, 4))
    start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return table, start, np.array(flags, dtype=np.uint8), P, R


def _channel_codes(ref_channels):
    """(codes 0..k-1 per region, sorted unique ``str(channel)``) — the keys of the reference's dicts."""
    names = [str(_ch) for _ch in ref_channels]
    uniq = [str(_u) for _u in np.unique(np.array(names))]
    if len(uniq) > L.PICK_MAX_CHANNELS:
        raise NotImplementedError("%d channels: at most %d are built" % (len(uniq), L.PICK_MAX_CHANNELS))
    return np.array([uniq.index(_n) for _n in names], dtype=np.int32), uniq


def upload_population(cand_hzxys_list, cand_ids=None, ref_ids=None, ref_channels=None):
    """A resident population (``_lib.PickPopulation``) of ragged ``cand_hzxys_list[chromosome][region]`` (``[]``, one 1-D
    row or a (k, 4) table of h, z, x, y in nm) with the ids and channels that the shims below would be given.  Not a
    reference name: hand it to them in place of the lists and nothing is uploaded again."""
    table, start, flags, P, R = _pack(cand_hzxys_list)
    codes, names = (None, []) if ref_channels is None else _channel_codes(ref_channels)
    if ref_channels is not None and len(ref_channels) != R:
        raise IndexError("wrong length of ref_channels, length should match the regions")
    pop = L.PickPopulation.upload(table, start, flags, P, R, codes, len(names))
    pop.cand_ids = np.arange(R) if cand_ids is None else np.array(cand_ids)
    pop.ref_ids = pop.cand_ids if ref_ids is None else np.array(ref_ids)
    pop.ref_channels = None if ref_channels is None else list(ref_channels)
    pop.channel_names = names
    pop.region_start, pop.row_1d = start, flags
    if len(pop.cand_ids) != R:
        raise IndexError("cand_hzxys should have same length as cand_ids")
    return pop


def _rows_population(P, R, ids, ref_ids, ref_channels):
    """A population without candidates: the carrier of picked / reference rows for the steps that read only those."""
    return upload_population([[[] for _r in range(R)] for _p in range(P)], ids, ref_ids, ref_channels)


def _windows(ids, ref_ids, neighbor_len, channels, split, needed=None):
    """CSR (offsets, indices) of the local windows (:1689-1699) of regions with ``ids`` against ``ref_ids``: the ids of
    ``[start, id) U (id, end)`` that are in ``ref_ids``, ascending, each as its first index in ``ref_ids``; with ``split``
    those of the region's channel, ascending by index.  The order is the order of ``np.nanmean``'s additions."""
    ref_list = [int(_v) for _v in ref_ids]
    first = {}
    for _k, _v in enumerate(ref_list):
        first.setdefault(_v, _k)
    lo_all, hi_all = min(ref_list), max(ref_list) + 1
    uniq = sorted(first)
    starts, idx = [0], []
    for _j, _id in enumerate(ids):
        _id = int(_id)
        _inds = []
        if needed is None or needed[_j]:
            _lo, _hi = max(_id - neighbor_len, lo_all), min(_id + neighbor_len + 1, hi_all)
            _inds = [first[_v] for _v in uniq[bisect.bisect_left(uniq, _lo):bisect.bisect_left(uniq, _hi)] if _v != _id]
            if split:
                if not _inds:   # np.intersect1d of an empty list is float64 and does not index (:1697-1699)
                    raise IndexError("arrays used as indices must be of integer (or boolean) type")
                _inds = sorted(_k for _k in _inds if channels[_k] == channels[_j])
        idx.extend(_inds)
        starts.append(len(idx))
    return np.array(starts, dtype=np.int32), np.array(idx, dtype=np.int32)


def _center_table(centers, P):
    """(P, 3) table of given chromosome centres (:1612-1631), or None when none is given."""
    if centers is None or all(_c is None for _c in centers):
        return None
    out = np.zeros((P, 3))
    for _p in range(P):
        _c = centers[_p]
        if _c is None:
            raise NotImplementedError("centres for some chromosomes only are not built: give all or none")
        if isinstance(_c, dict):
            raise NotImplementedError("ref_center as a dict does nothing in the reference (:1628-1629) and is not built")
        if not isinstance(_c, (list, np.ndarray)):
            raise TypeError("Wrong input type for ref_center: %s" % type(_c))
        if len(_c) > 3:
            out[_p] = np.array(_c)[1:4]
        elif len(_c) == 3:
            out[_p] = np.array(_c)
        else:
            raise IndexError("ref_center should at least have 3 elements")
    return out


def _split_regions(flat, pop, one_d_scalar=True, empty=None):
    """Per chromosome and region the slice of a per-candidate array: ``empty()`` for an empty region, a scalar for a 1-D
    row, an array for a table."""
    out = []
    for _p in range(pop.P):
        regs = []
        for _r in range(pop.R):
            _e = _p * pop.R + _r
            _a, _b = pop.region_start[_e], pop.region_start[_e + 1]
            if _a == _b:
                regs.append([] if empty is None else empty())
            elif pop.row_1d[_e] and one_d_scalar:
                regs.append(flat[_a])
            else:
                regs.append(flat[_a:_b].copy())
        out.append(regs)
    return out


def pick_spots_by_intensities(cand_spot_list, pix_size=_distance_zxy):
    """picking.py:1723-1749 — (P, R, 4) array: per chromosome and region the first candidate of maximal h
    (``np.argmax``: the first NaN wins), a NaN row for an empty region.  Tables with more than four columns are cut to
    (h, z, x, y) and scaled by ``pix_size``.  ``cand_spot_list``: ragged lists or a resident ``PickPopulation``.  An entry
    given as a 1-D row raises IndexError, as in the reference (``np.shape(_spots)[1]``)."""
    if isinstance(cand_spot_list, L.PickPopulation):
        pop = cand_spot_list
        if pop.row_1d.any():
            raise IndexError("tuple index out of range")
        pop.pick_by_intensity()
        return pop.download(L.PICK_GET_PICKS)
    lists = []
    for _spot_list in cand_spot_list:
        regs = []
        for _spots in _spot_list:
            if len(_spots) == 0:
                regs.append([])
                continue
            _spots = np.array(_spots)
            if np.shape(_spots)[1] == 4:
                regs.append(_spots)
            else:
                _hzxys = np.array(_spots)[:, :4]
                _hzxys[:, 1:4] = _hzxys[:, 1:4] * np.array(pix_size)[np.newaxis, :]
                regs.append(_hzxys)
        lists.append(regs)
    with upload_population(lists) as pop:
        pop.pick_by_intensity()
        return pop.download(L.PICK_GET_PICKS)


def _check_channels(split_channels, ref_channels, n):
    if split_channels and ref_channels is None:
        raise ValueError("ref_channels should be given if split_channels is True")
    if ref_channels is not None and len(ref_channels) != n:
        raise ValueError("ref_channels should have the same length as cand_hzxys")


def chromosome_center_dists(cand_hzxys, ref_center=None, split_channels=False, ref_channels=None):
    """picking.py:1578-1656 — per region of ONE chromosome the distance of its candidates to the chromosome centre:
    ``np.array([nan])`` for an empty region, a scalar for a 1-D row (BLAS norm), an array for a table.  The centre is
    ``ref_center`` (3 values, or more with z, x, y at 1:4) or ``np.nanmean`` of all candidates, per channel with
    ``split_channels``.  ``ref_center`` as a dict is not built (NotImplementedError): in the reference it leaves the centre
    unset."""
    _check_channels(split_channels, ref_channels, len(cand_hzxys))
    if isinstance(ref_center, dict):
        raise NotImplementedError("ref_center as a dict does nothing in the reference (:1628-1629) and is not built")
    ctr = _center_table([ref_center], 1)
    R = len(cand_hzxys)
    with upload_population([list(cand_hzxys)], None, None, ref_channels if split_channels else None) as pop:
        ws, wi = np.zeros(R + 1, dtype=np.int32), np.zeros(0, dtype=np.int32)
        pop.scores(ws, wi, split_dist=split_channels, centers=ctr, dist_only=True)
        d = pop.download(L.PICK_GET_CAND_DISTS)[:, 0]
        return _split_regions(d, pop, empty=lambda: np.array([np.nan]))[0]


def local_center_dists(cand_hzxys, cand_ids, ref_hzxys, ref_ids=None, neighbor_len=5, split_channels=False,
                       ref_channels=None):
    """picking.py:1658-1720 — per region of ONE chromosome the distance of its candidates to the mean of the reference
    rows within ``neighbor_len`` ids (the region's own id left out; of its channel with ``split_channels``): ``[]`` for
    an empty region, a scalar for a 1-D row, an array for a table; NaN where the window holds no number.  An integer
    ``cand_ids`` raises AttributeError as in the reference (``np.int``)."""
    _check_channels(split_channels, ref_channels, len(cand_hzxys))
    if cand_ids is None:
        cand_ids = np.arange(len(cand_hzxys))
    if isinstance(cand_ids, (int, np.int32)):
        raise AttributeError("module 'numpy' has no attribute 'int'")
    if len(cand_hzxys) != len(cand_ids):
        raise IndexError("cand_hzxys should have same length as cand_ids")
    if ref_ids is None:
        ref_ids = np.arange(len(ref_hzxys))
    if len(ref_hzxys) != len(ref_ids):
        raise IndexError("ref_hzxys should have same length as ref_ids")
    if len(ref_ids) != len(cand_ids):
        raise NotImplementedError("reference rows of another length than the regions are not built")
    needed = [len(_e) > 0 for _e in cand_hzxys]
    ws, wi = _windows(cand_ids, ref_ids, neighbor_len, ref_channels, split_channels, needed)
    with upload_population([list(cand_hzxys)], cand_ids, ref_ids, None) as pop:
        pop.set_rows(L.PICK_ROWS_REF, np.array(ref_hzxys, dtype=np.float64)[np.newaxis])
        pop.scores(ws, wi, ref_is_picks=False, dist_only=True)
        d = pop.download(L.PICK_GET_CAND_DISTS)[:, 1]
        return _split_regions(d, pop)[0]


def _run_e_step(pop, picked_ids, neighbor_len, split_channels, ref_chr_cts, ref_is_picks, windows=None):
    ws, wi = windows or _windows(picked_ids, pop.ref_ids, neighbor_len, pop.ref_channels, split_channels)
    pop.reference(ws, wi, split=split_channels, centers=_center_table(ref_chr_cts, pop.P), ref_is_picks=ref_is_picks)


def _reference_dicts(pop, split_channels):
    out = []
    for _kind in range(3):
        d = {}
        if split_channels:
            for _k, _name in enumerate(pop.channel_names):
                d[_name] = pop.sorted_reference(_kind, _k)
        d["all"] = pop.sorted_reference(_kind, pop.n_channels)
        out.append(d)
    return out[0], out[1], out[2]


def generate_reference_from_population(picked_hzxys_list, picked_ids=None, ref_hzxys_list=None, ref_ids=None,
                                       ref_channels=None, ref_chr_cts=None, parallel=True, num_threads=12,
                                       neighbor_len=7, collapse_regions=True, split_channels=True, sort=True,
                                       verbose=True):
    """picking.py:1768-1876, the E-step — three dicts (centre distances, local-centre distances, intensities) of the picked
    rows of a population, keyed ``'all'`` and, with ``split_channels``, ``str(channel)``; NaNs dropped, sorted with
    ``sort``.  ``picked_hzxys_list``: (P, R, 4) rows, or a resident ``PickPopulation`` whose current picks are meant.
    ``parallel`` / ``num_threads`` start no pool: they change the printed line only.  ``collapse_regions=False`` fails
    in the reference (:1863 unpacks an int): NotImplementedError here."""
    if verbose:
        print("-- generate reference metrics")
    resident = isinstance(picked_hzxys_list, L.PickPopulation)
    R = picked_hzxys_list.R if resident else len(picked_hzxys_list[0])
    if picked_ids is None:
        picked_ids = picked_hzxys_list.cand_ids if resident else np.arange(R)
    if ref_ids is None:
        ref_ids = picked_ids
    if resident and ref_channels is None:
        ref_channels = picked_hzxys_list.ref_channels
    if split_channels and ref_channels is None:
        raise ValueError("ref_channels should be given if split_channels is True")
    if ref_channels is not None and len(ref_channels) != len(picked_ids):
        raise IndexError("wrong length of ref_channels, length should match picked_ids")
    if not collapse_regions:
        raise NotImplementedError("collapse_regions=False fails in the reference (:1863) and is not built")
    if len(ref_ids) != R:
        raise NotImplementedError("reference rows of another length than the regions are not built")
    _t0 = time.time()
    if verbose:
        if parallel and num_threads > 1:
            print("--- multiprocessing expectation step with %s threads" % num_threads, end=', ')
        else:
            print("--- expectation step", end=', ')
    if resident:
        pop, own = picked_hzxys_list, False
        if ref_hzxys_list is not None:
            pop.set_rows(L.PICK_ROWS_REF, ref_hzxys_list)
    else:
        picked = np.array(picked_hzxys_list, dtype=np.float64)
        pop, own = _rows_population(picked.shape[0], R, picked_ids, ref_ids, ref_channels), True
        pop.set_rows(L.PICK_ROWS_PICKS, picked)
        if ref_hzxys_list is not None and ref_hzxys_list is not picked_hzxys_list:
            pop.set_rows(L.PICK_ROWS_REF, np.array(ref_hzxys_list, dtype=np.float64))
    try:
        same = ref_hzxys_list is None or ref_hzxys_list is picked_hzxys_list
        split = bool(split_channels) and ref_channels is not None
        _run_e_step(pop, picked_ids, neighbor_len, split, ref_chr_cts, same)
        if verbose:
            print("in %.3fs" % (time.time() - _t0))
            print("--- collapse all regions into 1d.")
        if sort:
            return _reference_dicts(pop, split)
        # unsorted: the arrays in the reference's order, collapsed from the per-region values on the host
        out = []
        codes = np.array([pop.channel_names.index(str(_c)) for _c in ref_channels]) if split else None
        for _what in (L.PICK_GET_REF_CT, L.PICK_GET_REF_LOCAL, L.PICK_GET_REF_INT):
            v, d = pop.download(_what), {}
            if split:
                for _k, _name in enumerate(pop.channel_names):
                    _v = v[:, np.where(codes == _k)[0]]
                    d[_name] = _v[~np.isnan(_v)]
                d["all"] = np.concatenate(list(d.values()))
            else:
                d["all"] = v[~np.isnan(v)]
            out.append(d)
        return out[0], out[1], out[2]
    finally:
        if own:
            pop.free()


def cum_val(sorted_vals, target, niter_max=15):
    """picking.py:1879-1899 — ``mid / len(sorted_vals)`` of the reference's bounded binary search for ``target`` (strict
    ``<``; at most 16 iterations; 0.5 in place of a ``mid`` of 0), searched on the device.  IndexError for an empty array."""
    if niter_max != L.PICK_NITER_MAX:
        raise NotImplementedError("niter_max other than %d is not built" % L.PICK_NITER_MAX)
    mid = int(L.cum_vals(sorted_vals, [target])[0])
    if mid == 0:
        mid += 0.5
    return mid / float(len(sorted_vals))


def slow_cum_val(ref_vals, target):
    """picking.py:1901-1903 — the share of the non-NaN ``ref_vals`` below ``target`` (host NumPy, as in the reference)."""
    return np.sum(np.array(ref_vals < target)[np.isnan(ref_vals) == False]) / np.sum(np.isnan(ref_vals) == False)   # noqa: E712


def _set_references(pop, ref_ct_dists, ref_local_dists, ref_ints, split_int, split_dist, center_weight, local_weight):
    """Upload the caller's reference dicts: the arrays that a score reads, found under the keys the reference uses
    (``ref_channels[region]`` as given, or ``'all'``; a missing key is the reference's KeyError)."""
    for _kind, (_d, _split) in enumerate(((ref_ct_dists, split_dist), (ref_local_dists, split_dist), (ref_ints, split_int))):
        if (_kind == 0 and center_weight == 0) or (_kind == 1 and local_weight == 0):
            continue
        if _split:
            done = set()
            for _ch in pop.ref_channels:
                _v, _key = _d[_ch], pop.channel_names.index(str(_ch))
                if _key not in done:
                    pop.set_sorted(_kind, _key, _v)
                    done.add(_key)
        else:
            pop.set_sorted(_kind, pop.n_channels, _d["all"])


def _m_windows(pop, neighbor_len, split_dist):
    needed = (np.diff(pop.region_start).reshape(pop.P, pop.R) > 0).any(axis=0)
    return _windows(pop.cand_ids, pop.ref_ids, neighbor_len, pop.ref_channels, split_dist, needed)


def _run_m_step(pop, neighbor_len, center_weight, local_weight, split_int, split_dist, ref_centers, ref_is_picks,
                windows=None):
    ws, wi = windows or _m_windows(pop, neighbor_len, split_dist)
    pop.scores(ws, wi, split_int=split_int, split_dist=split_dist, center_weight=center_weight, local_weight=local_weight,
               centers=_center_table(ref_centers, pop.P), ref_is_picks=ref_is_picks)


def pick_spots_by_scores(cand_hzxys_list, cand_ids=None, ref_channels=None, ref_hzxys_list=None, ref_ids=None,
                         ref_centers=None, ref_ct_dists=None, ref_local_dists=None, ref_ints=None, ref_chr_cts=None,
                         parallel=True, num_threads=12, neighbor_len=7, center_weight=1., local_weight=1.,
                         pix_size=_distance_zxy, collapse_regions=True, split_intensity_channels=False,
                         split_distance_channels=False, return_other_scores=False, sort=True, verbose=True):
    """picking.py:2017-2134, the M-step — per chromosome the selected rows ((R, 4), NaN for an empty region), their scores
    ((R,), ``np.nanmax`` of the region) and all scores (per region ``[]``, a scalar or an array); with
    ``return_other_scores`` also the scores that differ from the selected one.  The score of a candidate is
    ``log(cum_val(ints)) + center_weight * log(1 - cum_val(ct)) + local_weight * log(1 - cum_val(local))``; the first
    candidate of maximal score is selected.  ``cand_hzxys_list``: ragged lists or a resident ``PickPopulation`` (its ids
    and channels are used; others given here raise ValueError).  On a resident population the call still follows the
    reference's contract and not an EM loop's: without ``ref_hzxys_list`` the population's current picks are REPLACED by the
    brightest candidates, a given ``ref_hzxys_list`` (P*R rows) and given reference dicts are uploaded by every call, and
    the results are downloaded.  A loop that moves nothing of that size is ``em_pick_spots``.
    Without ``ref_hzxys_list`` the brightest candidates are the reference
    rows; without all three reference dicts the E-step makes them from the reference rows.

    As in the reference: without reference dicts and without a split flag ``split_channels`` is unset (:2051-2067) and
    UnboundLocalError is raised; ``parallel`` / ``num_threads`` start no pool and change the printed line only;
    ``collapse_regions=False`` is NotImplementedError (:1863); a ``ref_centers`` entry as a dict is NotImplementedError;
    ``return_other_scores`` with a region given as ONE 1-D row is TypeError (:2126 takes ``len()`` of its scalar score)."""
    if verbose:
        print("- pick spots by scores")
    resident = isinstance(cand_hzxys_list, L.PickPopulation)
    if resident:
        pop = cand_hzxys_list
        _same = lambda _a, _b: len(_a) == len(_b) and all(_x == _y for _x, _y in zip(_a, _b))   # noqa: E731
        if cand_ids is not None and not _same(cand_ids, pop.cand_ids):
            raise ValueError("cand_ids differ from those the resident population was uploaded with")
        if ref_ids is not None and not _same(ref_ids, pop.ref_ids):
            raise ValueError("ref_ids differ from those the resident population was uploaded with")
        if ref_channels is not None and (pop.ref_channels is None or not _same(ref_channels, pop.ref_channels)):
            raise ValueError("ref_channels differ from those the resident population was uploaded with")
        cand_ids, ref_channels = pop.cand_ids, pop.ref_channels
    if cand_ids is None:
        cand_ids = np.arange(len(cand_hzxys_list[0]))
    if ref_channels is None and split_intensity_channels:
        raise ValueError("split_intensity_channels is turned on but ref_channels are not given, exit")
    if ref_channels is None and split_distance_channels:
        raise ValueError("split_distance_channels is turned on but ref_channels are not given, exit")
    if not collapse_regions:
        raise NotImplementedError("collapse_regions=False fails in the reference (:1863) and is not built")
    have_refs = not (ref_ints is None or ref_ct_dists is None or ref_local_dists is None)
    split_any = bool(split_distance_channels or split_intensity_channels)
    own = not resident
    if ref_hzxys_list is None and verbose:
        print("-- reference pick not given, try to initiate by max-intensity pick")
    if not have_refs and not split_any:
        raise UnboundLocalError("local variable 'split_channels' referenced before assignment")
    if own:
        pop = upload_population(cand_hzxys_list, cand_ids, ref_ids, ref_channels)
    try:
        if ref_hzxys_list is None:
            if pop.row_1d.any():
                raise IndexError("tuple index out of range")
            pop.pick_by_intensity()
        else:
            pop.set_rows(L.PICK_ROWS_PICKS, np.array(ref_hzxys_list, dtype=np.float64))
        if not have_refs:
            generate_reference_from_population(pop, pop.ref_ids, None, pop.ref_ids, ref_chr_cts=ref_chr_cts,
                                               ref_channels=ref_channels, parallel=parallel, num_threads=num_threads,
                                               neighbor_len=neighbor_len, collapse_regions=collapse_regions,
                                               split_channels=True, sort=sort, verbose=verbose)
        else:
            _set_references(pop, ref_ct_dists, ref_local_dists, ref_ints, split_intensity_channels, split_distance_channels,
                            center_weight, local_weight)
        _t0 = time.time()
        if verbose:
            if parallel:
                print("--- multiprocessing maximization step with %d threads" % int(num_threads), end=', ')
            else:
                print("--- maximization step", end=', ')
        _run_m_step(pop, neighbor_len, center_weight, local_weight, bool(split_intensity_channels),
                    bool(split_distance_channels), ref_centers, True)
        sel = pop.download(L.PICK_GET_PICKS)
        sel_scores = pop.download(L.PICK_GET_SEL_SCORES)
        all_scores_list = _split_regions(pop.download(L.PICK_GET_SCORES), pop)
        if verbose:
            print("in %.3fs" % (time.time() - _t0))
    finally:
        if own:
            pop.free()
    sel_hzxys_list = [sel[_p] for _p in range(len(sel))]
    sel_scores_list = [sel_scores[_p] for _p in range(len(sel))]
    if not return_other_scores:
        return sel_hzxys_list, sel_scores_list, all_scores_list
    other_scores_list = []
    for _sel_scores, _all_scores in zip(sel_scores_list, all_scores_list):
        _other_scores = []
        for _s, _scs in zip(_sel_scores, _all_scores):
            if np.isnan(_s).sum() > 0:
                _other_scores.append(_scs)
            elif len(_scs) == 0:
                _other_scores.append(np.array([]))
            else:
                _other_scores.append(_scs[_scs != _s])
        other_scores_list.append(_other_scores)
    return sel_hzxys_list, sel_scores_list, all_scores_list, other_scores_list


def EM_pick_scores_in_population(*args, **kwargs):
    """picking.py:2137-2278 is the superseded form (it imports ``tqdm.notebook`` and multiplies un-logged values) and is
    not built: use ``pick_spots_by_scores`` or ``em_pick_spots``."""
    raise NotImplementedError("EM_pick_scores_in_population is superseded in the reference and not built; "
                              "use pick_spots_by_scores or em_pick_spots")


def evaluate_differences(old_hzxys_list, new_hzxys_list=None):
    """picking.py:2280-2284 — the share of rows whose z, x, y moved by less than 0.01 among the rows whose distance is not
    NaN, counted on the device.  A resident ``PickPopulation`` as the only argument compares its previous and its
    current picks."""
    if isinstance(old_hzxys_list, L.PickPopulation):
        near, num = old_hzxys_list.difference()
    else:
        old = np.array(old_hzxys_list, dtype=np.float64)
        new = np.array(new_hzxys_list, dtype=np.float64)
        with _rows_population(old.shape[0], old.shape[1], None, None, None) as pop:
            pop.set_rows(L.PICK_ROWS_PREV, old)
            pop.set_rows(L.PICK_ROWS_PICKS, new)
            near, num = pop.difference()
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.int64(near) / np.int64(num)


def em_pick_spots(population_or_lists, n_iter_max=10, stop_ratio=0.99, cand_ids=None, ref_channels=None, neighbor_len=7,
                  center_weight=1., local_weight=1., split_intensity_channels=False, split_distance_channels=False,
                  ref_centers=None, verbose=False):
    """NOT a reference name: the loop that the reference's users write around the population picker, run on a resident
    population.  Start from ``pick_spots_by_intensities``; per iteration the E-step on the current picks
    (``generate_reference_from_population``, channels split when either split flag is set), the M-step with the current
    picks as reference rows (``pick_spots_by_scores``) and ``evaluate_differences`` of the old and new picks; stop when
    that ratio reaches ``stop_ratio`` or after ``n_iter_max`` iterations.  Per iteration the host reads the lengths of the
    reference arrays and the 8-byte difference record; the population is not uploaded again.

    Returns ((P, R, 4) picks, (P, R) scores, list of the ratio per iteration)."""
    own = not isinstance(population_or_lists, L.PickPopulation)
    pop = upload_population(population_or_lists, cand_ids, None, ref_channels) if own else population_or_lists
    try:
        split_int, split_dist = bool(split_intensity_channels), bool(split_distance_channels)
        if (split_int or split_dist) and pop.ref_channels is None:
            raise ValueError("a split flag is turned on but ref_channels are not given, exit")
        if pop.row_1d.any():
            raise IndexError("tuple index out of range")   # pick_spots_by_intensities on a 1-D entry
        pop.pick_by_intensity()
        ratios = []
        e_win = _windows(pop.ref_ids, pop.ref_ids, neighbor_len, pop.ref_channels, split_int or split_dist)
        m_win = _m_windows(pop, neighbor_len, split_dist)
        for _it in range(int(n_iter_max)):
            _run_e_step(pop, pop.ref_ids, neighbor_len, split_int or split_dist, None, True, e_win)
            _run_m_step(pop, neighbor_len, center_weight, local_weight, split_int, split_dist, ref_centers, True, m_win)
            ratios.append(evaluate_differences(pop))
            if verbose:
                print("-- iteration %d, similarity %.4f" % (_it, ratios[-1]))
            if ratios[-1] >= stop_ratio:
                break
        return pop.download(L.PICK_GET_PICKS), pop.download(L.PICK_GET_SEL_SCORES), ratios
    finally:
        if own:
            pop.free()


# ---- the per-cell pickers (:14-64, :662-765, :797-1563) ------------------------------------------------------------------------

def _bad_spot(width):
    _b = np.ones(width) * np.nan
    _b[0] = 0
    return _b


def _upload_cells(cells, distance_zxy):
    """A ``CellPickPopulation`` of ``cells`` with its per-cell host state; the caller's lists are not copied."""
    pop = L.CellPickPopulation.upload([(_c[0], _c[1], _c[2]) for _c in cells], (1, 1, 1) if distance_zxy is None else distance_zxy)
    pop.cells = cells
    return pop


def _merge(pop, intensity_th, hard_intensity_th, dist_th=0.1):
    pop.merge(intensity_th, hard_intensity_th, dist_th)
    pop._merged_cache = {}
    pop._naive_cache = {}
    pop._planned = False
    pop._spop = None


def _cell_merged(pop, k):
    """merge_spot_list of every region of cell k, in the caller's region order."""
    if k not in pop._merged_cache:
        pop._merged_cache[k] = [pop.merged_region(_g) for _g in range(pop.region_start[k], pop.region_start[k + 1])]
    return pop._merged_cache[k]


def population_merge_spot_lists(cells, dist_th=0.1, dist_norm=2, intensity_th=0., hard_intensity_th=True):
    """NOT a reference name.  ``[merge_spot_list(spot_list, ..., append_nan_spots=chrom_coords is not None,
    chrom_coords=chrom_coords) for spot_list in cell_cand_spots]`` of every cell ``(cell_cand_spots, region_ids,
    chrom_coords)``, merged on the device in one call."""
    if dist_norm != 2:
        raise NotImplementedError("merge_spot_list: dist_norm %s is not built (2, the Euclidean norm, is)" % (dist_norm,))
    with _upload_cells(cells, None) as pop:
        _merge(pop, intensity_th, hard_intensity_th, dist_th)
        return [_cell_merged(pop, _k) for _k in range(pop.n_cells)]


def merge_spot_list(spot_list, dist_th=0.1, dist_norm=2,
                    intensity_th=0., hard_intensity_th=True,
                    append_nan_spots=False, chrom_coords=None):
    """picking.py:662-765 — the spots of ``spot_list`` (one table per chromosome) without those within ``dist_th`` pixels of
    an earlier kept spot and, with ``intensity_th``, without the dim ones (``hard_intensity_th=False`` keeps at least
    ``len(spot_list)`` of the brightest); with ``append_nan_spots`` a placeholder row (0, chromosome coordinate, NaN ...)
    stands for every chromosome that has no list and is appended for every chromosome that owns no kept spot."""
    if append_nan_spots and chrom_coords is None:
        raise ValueError(f"chrom_coords should be given if append_nan_spots is True")
    if dist_norm != 2:
        raise NotImplementedError("merge_spot_list: dist_norm %s is not built (2, the Euclidean norm, is)" % (dist_norm,))
    if len(spot_list) == 0 or (not append_nan_spots and all(len(_s) == 0 for _s in spot_list)):
        if append_nan_spots:
            raise NotImplementedError("merge_spot_list: no spot list with append_nan_spots fails in the reference (:749) and is not built")
        return np.array([])
    return population_merge_spot_lists([([spot_list], [0], chrom_coords if append_nan_spots else None)], dist_th, dist_norm,
                                       intensity_th, hard_intensity_th)[0][0]


def _naive_own(lists):
    """Per entry of ``lists`` (a table of spots or empty) the place of the brightest spot by the pinned argsort, -1 for an
    empty entry, picked on the device."""
    if len(lists) == 0:
        return np.zeros(0, dtype=int)
    with _upload_cells([([[_l] for _l in lists], np.arange(len(lists)), None)], None) as pop:
        pick, _ = pop.naive(L.IA3_CELLPICK_NAIVE_OWN)
        return np.where(pick[:, 0] < 0, -1, pick[:, 0] - pop.cand_start[:-1:L.IA3_CELLPICK_MAX_CHROM])


def naive_pick_spots(cand_spots, region_ids, use_chrom_coord=True, chrom_id=None,
                     return_indices=False, verbose=True):
    """picking.py:14-64 — Naive pick spots simply by intensity."""
    if len(cand_spots) != len(region_ids):
        raise ValueError(
            "cand_spots and region_ids should have the same length!")
    if chrom_id is None and use_chrom_coord:
        raise ValueError(
            f"chrom_id should be given if use_chrom_coord is True!")
    elif chrom_id is not None and not isinstance(chrom_id, int):
        chrom_id = int(chrom_id)
    _lists = []
    for _spots, _id in zip(cand_spots, region_ids):
        if use_chrom_coord:
            if len(_spots) <= chrom_id:
                raise IndexError(
                    f" spots:{_spots} for region:{_id} doesn't have spots for chromosome {chrom_id}")
            _lists.append(np.array(_spots[chrom_id]))
        else:
            _lists.append(np.array(_spots))
    _inds = _naive_own(_lists)
    _selected_spots = []
    for _pts, _ind in zip(_lists, _inds):
        if _ind < 0:
            _bad_pt = np.nan * np.ones(11)
            if not use_chrom_coord:
                _bad_pt[0] = 0
            _selected_spots.append(_bad_pt)
        else:
            _selected_spots.append(_pts[_ind])
    if return_indices:
        return np.array(_selected_spots), np.array(_inds, dtype=int)
    else:
        return np.array(_selected_spots)


def _naive_cell(pop, k, chrom_share_spots, distance_zxy):
    """naive_pick_spots_for_chromosomes (:834-892) of cell k of a merged population: (_sel_spot_list, _sel_spot_inds)."""
    cell_cand_spots, region_ids, chrom_coords = pop.cells[k][:3]
    _merged_spot_list = _cell_merged(pop, k)
    _num_chroms = int(pop.n_chrom[k])
    _spot_obj_len = [np.array(_s[0]).shape[1] for _s in cell_cand_spots if len(_s) > 0 and len(_s[0]) > 0]
    if len(_spot_obj_len) == 0:
        _spot_obj_len = 11
    elif len(np.unique(_spot_obj_len)) == 1:
        _spot_obj_len = np.unique(_spot_obj_len)[0]
    else:
        raise ValueError(f"_spot object length is not unique, exit")
    _bad = _bad_spot(_spot_obj_len)
    g0, g1 = pop.region_start[k], pop.region_start[k + 1]
    if chrom_coords is None or chrom_share_spots:
        if L.IA3_CELLPICK_NAIVE_OWN not in pop._naive_cache:
            pop._naive_cache[L.IA3_CELLPICK_NAIVE_OWN] = pop.naive(L.IA3_CELLPICK_NAIVE_OWN)
        pick = pop._naive_cache[L.IA3_CELLPICK_NAIVE_OWN][0][g0:g1]
        _sel_spot_list = [np.array([pop.cell_rows[k][_p - pop.cell_cand0[k]] if _p >= 0 else np.nan * np.ones(11) for _p in pick[:, _i]])
                          for _i in range(_num_chroms)]
        _sel_spot_inds = [-1 * np.ones(len(_merged_spot_list), dtype=int) for _i in range(_num_chroms)]
    else:
        distance_zxy[np.newaxis, :]                   # :870 refuses a list, the package's default included
        if L.IA3_CELLPICK_NAIVE_MERGED not in pop._naive_cache:
            pop._naive_cache[L.IA3_CELLPICK_NAIVE_MERGED] = pop.naive(L.IA3_CELLPICK_NAIVE_MERGED)
        pick, sub = pop._naive_cache[L.IA3_CELLPICK_NAIVE_MERGED]
        _sel_spot_list = [[] for _i in range(_num_chroms)]
        _sel_spot_inds = [[] for _i in range(_num_chroms)]
        for _r, _spots in enumerate(_merged_spot_list):
            for _chrom_id in range(_num_chroms):
                _p = pick[g0 + _r, _chrom_id]
                if len(_spots) == 0 or _p < 0:
                    _sel_spot_list[_chrom_id].append(_bad.copy())
                    _sel_spot_inds[_chrom_id].append(-1)
                else:
                    _sel_spot_list[_chrom_id].append(_spots[_p])
                    _sel_spot_inds[_chrom_id].append(int(sub[g0 + _r, _chrom_id]))
        _sel_spot_list = [np.array(_spots) for _spots in _sel_spot_list]
        _sel_spot_inds = [np.array(_inds) for _inds in _sel_spot_inds]
    return _sel_spot_list, _sel_spot_inds


def _check_cells(cells):
    """What is refused before anything is uploaded; the number of chromosomes of every cell."""
    nums = []
    for _cand, _ids, _coords in [_c[:3] for _c in cells]:
        _n = len(_coords) if _coords is not None else len(_cand[0])
        if _n > L.IA3_CELLPICK_MAX_CHROM:
            raise NotImplementedError("%d chromosomes in a cell: at most %d are picked together (a spot of the next region walks "
                                      "up to C^C index tuples)" % (_n, L.IA3_CELLPICK_MAX_CHROM))
        nums.append(_n)
    return nums


def population_naive_pick_spots(cells, intensity_th=0., hard_intensity_th=True, chrom_share_spots=False,
                                distance_zxy=_distance_zxy, return_indices=False, verbose=True):
    """NOT a reference name.  ``naive_pick_spots_for_chromosomes`` of every cell ``(cell_cand_spots, region_ids,
    chrom_coords)``: a list with, per cell, what the reference returns for it."""
    nums = _check_cells(cells)
    out = [None] * len(cells)
    live = [_k for _k, _n in enumerate(nums) if _n > 0]
    for _k, _n in enumerate(nums):
        if _n == 0:
            out[_k] = ([], []) if return_indices else []
    if live:
        with _upload_cells([cells[_k] for _k in live], (1, 1, 1) if isinstance(distance_zxy, list) else distance_zxy) as pop:
            _merge(pop, intensity_th, hard_intensity_th)
            for _j, _k in enumerate(live):
                _spots, _inds = _naive_cell(pop, _j, chrom_share_spots, distance_zxy)
                out[_k] = (_spots, _inds) if return_indices else _spots
    return out


def naive_pick_spots_for_chromosomes(cell_cand_spots, region_ids, chrom_coords=None,
                                     intensity_th=0., hard_intensity_th=True,
                                     chrom_share_spots=False, distance_zxy=_distance_zxy,
                                     return_indices=False, verbose=True):
    """picking.py:797-899 — per chromosome the brightest spot of every region: among its own candidates without
    ``chrom_coords`` or with ``chrom_share_spots`` (all indices are -1 then, as in the reference), else among the merged
    spots nearest to its coordinate (the index counts within those, :885-888)."""
    return population_naive_pick_spots([(cell_cand_spots, region_ids, chrom_coords)], intensity_th, hard_intensity_th,
                                       chrom_share_spots, distance_zxy, return_indices, verbose)[0]


def _index_tuples(allowed, chrom_share_spots):
    """The tuples (one index per chromosome) of ``itertools.product`` over the chromosomes' allowed indices, in its order;
    unless spots are shared, only those whose indices all differ."""
    tuples = itertools.product(*allowed)
    if chrom_share_spots:
        return list(tuples)
    return [t for t in tuples if len(set(t)) == len(t)]


def _check_score_list(_score_list):
    if len(_score_list) == 0:
        raise ValueError(f"_score_list is empty, exit!")
    if len(_score_list[0]) == 0:
        raise ValueError(f"_score_list[0] is empty, no spots, exit!")
    return len(_score_list), len(_score_list[0])


def _all_score_combinations(_score_list, chrom_share_spots=False):
    """picking.py:1552-1563 — every tuple of spot indices, one per chromosome.  A host function: the device walks the
    same tuples in ``cp_pick`` (csrc/ia3_cellpick.h)."""
    C, K = _check_score_list(_score_list)
    return _index_tuples([np.arange(K)] * C, chrom_share_spots)


def _optimized_score_combinations(_score_list, chrom_share_spots=False):
    """picking.py:1531-1550 — the tuples over each chromosome's C best-scored indices (ascending by score, equal scores by
    ascending index: the tie rule of this module), or over all indices of a chromosome whose scores are all infinite."""
    C, K = _check_score_list(_score_list)
    if K < C:
        raise IndexError(f"there should be more spots than chromosomes!")
    allowed = [np.arange(K) if np.isinf(sc).all() else np.argsort(sc, kind='stable')[K - C:] for sc in _score_list]
    return _index_tuples(allowed, chrom_share_spots)


def _plan(pop):
    """The regions each cell's forward pass walks (:1066-1085): those with a merged spot without NaN, by ascending id
    (equal ids in the caller's order)."""
    if (pop.mcount > L.IA3_CELLPICK_MAX_SPOTS).any():
        raise NotImplementedError("%d merged spots in one region: at most %d are built (the spots of a region are the lanes of "
                                  "one wavefront)" % (pop.mcount.max(), L.IA3_CELLPICK_MAX_SPOTS))
    pop.order, pop.vpos, vstart, vreg, vgap = [], [], [0], [], []
    for _k in range(pop.n_cells):
        _ids = pop.region_ids[_k]
        _order = np.argsort(_ids, kind='stable')
        _g = pop.region_start[_k] + _order
        _valid = np.where((pop.mcount[_g] > 0) & (pop.mvalid[_g] > 0))[0]
        pop.order.append(_order)
        pop.vpos.append(_valid)                         # _id_indices
        vreg.extend(_g[_valid].tolist())
        _vid = _ids[_order][_valid]
        vgap.extend(([0] + np.diff(_vid).tolist()) if len(_vid) else [])
        vstart.append(len(vreg))
    pop.vstart = np.array(vstart)
    pop.vreg = np.array(vreg, dtype=np.int64)
    pop.plan(vstart, vreg, vgap)
    pop._planned = True


def _spot_scores(spop, score_metric, ref_metric, intensity_th, local_size, weights, distance_limits, nan_mask, inf_mask, ignore_nan):
    """Per chromosome of a ScorePopulation what ``generate_ref_from_chromosome`` returns for its selected spots and the sum
    ct + lc + int of ``spot_score_in_chromosome`` (:306-407) of its candidates against them."""
    arrays, counts, scalars = spop.references(ref_metric, local_size, intensity_th, ignore_nan)
    w = [float(weights[0]), float(weights[1]), 0., float(weights[2])]
    val, cls, ref_counts = spop.scores(score_metric, ref_metric, local_size, intensity_th, ignore_nan, w, distance_limits)
    if score_metric == 'cdf':
        for a in range(2):
            if w[a] != 0. and (ref_counts[:, a] == 0).any():
                raise ValueError(f"Wrong input ref_dist, not enough values to calculate cdf")
        if (ref_counts[:, 3] == 0).any():
            raise ValueError(f"Wrong input data, no valid points at all.")
    from .scoring import _finish, _reference_values, _say_fallbacks
    total = None
    for a in (0, 1, 3):
        s = _finish(val[a], cls[a], w[a], val[a].shape)
        if a < 3:
            if w[a] == 0.:
                s = np.zeros(s.shape)
            else:
                s[(cls[a] & L.SCORE_NAN_IN) != 0] = nan_mask
        else:
            s[np.isnan(s)] = nan_mask
            s[np.isinf(s)] = inf_mask
        total = s if total is None else total + s
    refs = []
    for c in range(spop.C):
        _say_fallbacks(counts[c])
        refs.append(_reference_values(arrays[c], counts[c], scalars[c], ref_metric, ignore_nan))
    at = spop.cand_start
    return refs, [total[at[c]:at[c + 1]] for c in range(spop.C)]


def _reference_ids(cell_cand_spots, region_ids, ref_spot_list, ref_spot_ids, spot_num_th):
    """The region id of every reference spot, per chromosome (:999-1025).  A chromosome with at least ``spot_num_th``
    reference spots keeps them, with ``ref_spot_ids``, the region ids when there is one spot per region, or 0 .. n-1.  One
    with fewer takes ALL its candidates as references -- written into ``ref_spot_list``, which the reference does too --
    each with the label of its region: ``ref_spot_ids`` when it has one entry per region, the region ids when it is not
    given, the region's position otherwise."""
    R = len(cell_cand_spots)
    if ref_spot_ids is None:
        labels = region_ids
    elif len(ref_spot_ids) == R:
        labels = ref_spot_ids
    else:
        labels = np.arange(R)
    ids = []
    for c in range(len(ref_spot_list)):
        n = len(ref_spot_list[c])
        if n >= spot_num_th:
            if ref_spot_ids is not None:
                ids.append(np.array(ref_spot_ids, dtype=int))
            else:
                ids.append(region_ids if n == len(region_ids) else np.arange(n))
            continue
        lists = [lists_r[c] for lists_r in cell_cand_spots]
        ref_spot_list[c] = np.concatenate(lists)
        ids.append(np.repeat(np.asarray(labels, dtype=np.float64)[:R], [len(t) for t in lists]))
    return ids


def _trace_back(pop, dy, ptr, walked, c):
    """The backward pass (:1158-1169) of chromosome c over the regions ``walked``: the first best dynamic score of the last
    region, then the stored pointers; the picked merged-spot index of every walked region."""
    at = pop.cap_start[walked]
    picks = np.empty(len(walked), dtype=int)
    picks[-1] = np.argmax(dy[c, at[-1]:at[-1] + pop.mcount[walked[-1]]])
    for j in range(len(walked) - 1, 0, -1):
        picks[j - 1] = ptr[c, at[j] + picks[j]]
    return picks


def _assemble(merged_sorted, order, walked_pos, picks, n_chrom):
    """What the dynamic picker returns for one cell (:1171-1194), in the caller's region order: per chromosome the picked
    spot and its index for the walked regions (a spot that holds a NaN -- a placeholder -- comes back as the bad spot but
    keeps its index), the bad spot and -1 for the others; tables of zeros when nothing was walked."""
    R, width = len(merged_sorted), merged_sorted[0].shape[1]
    spots = [np.zeros((R, width)) for _c in range(n_chrom)]
    inds = [np.full(R, -1, dtype=int) for _c in range(n_chrom)]
    for c in range(len(picks)):
        rows = [merged_sorted[j][i] for j, i in zip(walked_pos, picks[c])]
        spots[c][:] = _bad_spot(len(rows[-1]))
        for j, i, row in zip(walked_pos, picks[c], rows):
            spots[c][order[j]] = _bad_spot(len(row)) if np.isnan(row).any() else row
            inds[c][order[j]] = i
    return spots, inds


def _dynamic_cells(pop, ks, sel_lists, ref_lists, ref_spot_ids, nb_dist_list, P):
    """dynamic_pick_spots_for_chromosomes (:958-1200) of the cells ``ks`` of a merged population, with the reference's
    bookkeeping per cell on the host, one E-step and one forward pass for all of them.  ``sel_lists[k]`` / ``ref_lists[k]``:
    the caller's sel_spot_list / ref_spot_list or None.  Returns {k: (_sel_spot_list, _sel_ind_list)}."""
    MC = L.IA3_CELLPICK_MAX_CHROM
    score_metric, ref_metric = P["score_metric"], P["ref_dist_metric"]
    if not pop._planned:
        _plan(pop)
    st = {}
    _t0 = time.time()
    cand_t, cand_i, sel_t, sel_i, ctrs, slots = [], [], [], [], [], []
    for k in ks:
        cell_cand_spots, region_ids, chrom_coords = pop.cells[k][:3]
        _merged = _cell_merged(pop, k)
        _order = np.argsort(region_ids, kind='stable')
        _merged_spot_list = [_merged[_id] for _id in _order]
        _num_chroms = int(pop.n_chrom[k])
        sel_spot_list = sel_lists.get(k)
        if sel_spot_list is None:
            if P["verbose"]:
                print(f"-- initiate dynamic picking by naive picking spots.")
            sel_spot_list, _ = _naive_cell(pop, k, P["chrom_share_spots"], P["distance_zxy"])
            for _chrom_id in range(_num_chroms):
                sel_spot_list[_chrom_id] = np.array([sel_spot_list[_chrom_id][_id] for _id in _order])
        if nb_dist_list is not None:
            raise IndexError(f"Length of nb_dist_list{len(nb_dist_list)} doesn't match length of sel_spot_list:{len(sel_spot_list)}")
        ref_spot_list = ref_lists.get(k)
        if ref_spot_list is None:
            ref_spot_list = sel_spot_list             # one list, as in the reference: what follows writes into it
        ref_id_list = _reference_ids(cell_cand_spots, region_ids, ref_spot_list, ref_spot_ids, P["spot_num_th"])
        P["distance_zxy"][np.newaxis, :]              # scoring.py:243 refuses a list, the package's default included
        g0, g1 = pop.region_start[k], pop.region_start[k + 1]
        m0, m1 = pop.mstart[g0], pop.mstart[g1]
        rows4 = pop._rows4[m0:m1]
        ids4 = pop.region_ids[k][pop.mregion[m0:m1] - g0]
        for _chrom_id, (_ref_spots, _ref_ids) in enumerate(zip(ref_spot_list, ref_id_list)):
            if chrom_coords is not None and not P["update_chrom_coords"]:
                _chrom_coord = chrom_coords[_chrom_id]
            else:
                _chrom_coord = None
            if len(_ref_ids) != len(_ref_spots):
                raise IndexError(f"chr:{_chrom_id}, Length of _ref_ids:{len(_ref_ids)} doesn't match length of _ref_spots:{len(_ref_spots)}")
            if any(len(_s) == 0 for _s in _merged_spot_list):
                raise IndexError("too many indices for array: array is 1-dimensional, but 2 were indexed")   # :346 on an empty region
            if pop.vstart[k + 1] == pop.vstart[k]:
                continue                              # no region is walked: the scores of this cell are never read
            if len(_ref_spots) == 0:
                raise NotImplementedError("chromosome %d has no reference spot at all, which is not built" % _chrom_id)
            cand_t.append(rows4)
            cand_i.append(ids4)
            sel_t.append(np.array(_ref_spots))
            sel_i.append(np.array(_ref_ids, dtype=int))
            ctrs.append(_chrom_coord)
            slots.append((k, _chrom_id))
        st[k] = (_merged_spot_list, _order, _num_chroms)
    # the E-step: references and scores of every (cell, chromosome) from one ScorePopulation
    _tm = P.get("timings")
    _t1 = time.time()
    if _tm is not None:
        _tm["host_before_s"] = _tm.get("host_before_s", 0.) + _t1 - _t0
    L.score_half(P["local_size"])
    key = tuple(slots)
    if not slots:
        refs, totals = [], []
    elif pop._spop is not None and pop._spop_key == key:
        pop._spop.replace_selected(sel_t, sel_i)
    else:
        if pop._spop is not None:
            pop._spop.free()
        pop._spop = L.ScorePopulation.upload(cand_t, cand_i, sel_t, sel_i, ctrs, P["distance_zxy"])
        pop._spop_key = key
    if slots:
        refs, totals = _spot_scores(pop._spop, score_metric, ref_metric, P["intensity_th"], P["local_size"],
                                    (P["w_ctdist"], P["w_lcdist"], P["w_int"]), P["distance_limits"], P["nan_mask"], P["inf_mask"], P["ignore_nan"])
    scores = np.zeros((pop.planes, pop.cap))
    nb = {}
    w_nb = float(P["w_nbdist"])
    for (k, c), _ref, _tot in zip(slots, refs, totals):
        g0, g1 = pop.region_start[k], pop.region_start[k + 1]
        scores[c, pop.mpos[pop.mstart[g0]:pop.mstart[g1]]] = _tot
        if w_nb == 0.:
            continue
        if score_metric == 'linear':
            nb[(k, c)] = float(_ref[2])
        else:
            from .scoring import _no_nan
            nb[(k, c)] = L.cellpick_cdf_table(_no_nan(_ref[2], f"Wrong input ref_dist, not enough values to calculate cdf"), w_nb,
                                              min(P["distance_limits"]), max(P["distance_limits"]))
    if score_metric == 'cdf' and w_nb == 0.:
        for _slot in slots:
            nb[_slot] = (np.zeros(1), np.zeros(2))
    # the forward pass (:1093-1155)
    _t2 = time.time()
    if _tm is not None:
        _tm["e_step_s"] = _tm.get("e_step_s", 0.) + _t2 - _t1
    walk = [k for k in ks if pop.vstart[k + 1] - pop.vstart[k] > 0]
    for k in walk:
        _v = pop.vreg[pop.vstart[k]:pop.vstart[k + 1]]
        if not P["chrom_share_spots"] and (pop.mcount[_v[:-1]] < pop.n_chrom[k]).any():
            raise ValueError(f"Not enough _inds combinations")
    if walk:
        dy, ptr, err = pop.forward(sorted(walk), scores, score_metric, nb, w_nb, max(P["distance_limits"]), P["nan_mask"],
                                   P["chrom_share_spots"])
        if (err == 1).any():
            raise ValueError(f"Not enough _inds combinations")
        if (err == 2).any():
            raise ValueError("attempt to get argmax of an empty sequence")
        if (err == 3).any():
            raise NotImplementedError("more than %d index tuples for one spot: every score of a chromosome is infinite, so all its "
                                      "spots are allowed, which is not walked" % L.IA3_CELLPICK_MAX_TUPLES)
    _t3 = time.time()
    if _tm is not None:
        _tm["forward_s"] = _tm.get("forward_s", 0.) + _t3 - _t2
    out = {}
    for k in ks:
        _merged_spot_list, _order, _num_chroms = st[k]
        _v = pop.vreg[pop.vstart[k]:pop.vstart[k + 1]]
        picks = [_trace_back(pop, dy, ptr, _v, _c) for _c in range(_num_chroms)] if len(_v) else []
        _sel_spot_list, _sel_ind_list = _assemble(_merged_spot_list, _order, pop.vpos[k], picks, _num_chroms)
        out[k] = (_sel_spot_list, _sel_ind_list)
    if _tm is not None:
        _tm["host_after_s"] = _tm.get("host_after_s", 0.) + time.time() - _t3
    return out


def _dynamic_params(ref_dist_metric, spot_num_th, intensity_th, score_metric, local_size, w_ctdist, w_lcdist, w_int, w_nbdist,
                    ignore_nan, nan_mask, inf_mask, update_chrom_coords, chrom_share_spots, distance_zxy, distance_limits, verbose):
    score_metric, ref_dist_metric = str(score_metric), str(ref_dist_metric)
    if (score_metric == 'cdf') != (ref_dist_metric.lower() == 'cdf') and score_metric in ('linear', 'cdf'):
        raise NotImplementedError("score_metric %r with ref_dist_metric %r is not built: 'cdf' scores take 'cdf' references and "
                                  "'linear' scores one number" % (score_metric, ref_dist_metric))
    return dict(ref_dist_metric=ref_dist_metric.lower(), spot_num_th=spot_num_th, intensity_th=intensity_th, score_metric=score_metric,
                local_size=local_size, w_ctdist=w_ctdist, w_lcdist=w_lcdist, w_int=w_int, w_nbdist=w_nbdist, ignore_nan=ignore_nan,
                nan_mask=nan_mask, inf_mask=inf_mask, update_chrom_coords=update_chrom_coords, chrom_share_spots=chrom_share_spots,
                distance_zxy=distance_zxy, distance_limits=distance_limits, verbose=verbose)


def _open_cells(pop_cells, distance_zxy, intensity_th, hard_intensity_th):
    pop = _upload_cells(pop_cells, (1, 1, 1) if isinstance(distance_zxy, list) else distance_zxy)
    try:
        _merge(pop, intensity_th, hard_intensity_th)
        pop._rows4 = pop.merged_rows4()
    except Exception:
        pop.free()
        raise
    return pop


def _close_cells(pop):
    if getattr(pop, "_spop", None) is not None:
        pop._spop.free()
    pop.free()


def population_dynamic_pick_spots(cells, ref_spot_ids=None, ref_dist_metric='median', nb_dist_list=None, spot_num_th=100,
                                  intensity_th=0., hard_intensity_th=True, ignore_region_ids=False, score_metric='linear',
                                  local_size=5, w_ctdist=2, w_lcdist=1, w_int=1, w_nbdist=2,
                                  ignore_nan=True, nan_mask=0., inf_mask=-1000.,
                                  update_chrom_coords=False, chrom_share_spots=False,
                                  distance_zxy=_distance_zxy, distance_limits=[200, 3000],
                                  return_indices=False, verbose=True):
    """NOT a reference name.  ``dynamic_pick_spots_for_chromosomes`` of every cell in one E-step and one forward pass.
    A cell is ``(cell_cand_spots, region_ids, chrom_coords)`` and may go on with ``sel_spot_list`` and ``ref_spot_list``
    (each a list per chromosome, or None).  Returns a list with, per cell, what the reference returns for it."""
    nums = _check_cells(cells)
    P = _dynamic_params(ref_dist_metric, spot_num_th, intensity_th, score_metric, local_size, w_ctdist, w_lcdist, w_int, w_nbdist,
                        ignore_nan, nan_mask, inf_mask, update_chrom_coords, chrom_share_spots, distance_zxy, distance_limits, verbose)
    out = [None] * len(cells)
    live = [_k for _k, _n in enumerate(nums) if _n > 0]
    for _k, _n in enumerate(nums):
        if _n == 0:
            out[_k] = ([], []) if return_indices else []
    if live:
        pop = _open_cells([cells[_k] for _k in live], distance_zxy, intensity_th, hard_intensity_th)
        try:
            sel = {_j: (cells[_k][3] if len(cells[_k]) > 3 else None) for _j, _k in enumerate(live)}
            ref = {_j: (cells[_k][4] if len(cells[_k]) > 4 else None) for _j, _k in enumerate(live)}
            got = _dynamic_cells(pop, list(range(len(live))), sel, ref, ref_spot_ids, nb_dist_list, P)
        finally:
            _close_cells(pop)
        for _j, _k in enumerate(live):
            out[_k] = got[_j] if return_indices else got[_j][0]
    return out


def dynamic_pick_spots_for_chromosomes(cell_cand_spots, region_ids,
                                       chrom_coords=None, sel_spot_list=None,
                                       ref_spot_list=None, ref_spot_ids=None,
                                       ref_dist_metric='median', nb_dist_list=None, spot_num_th=100,
                                       intensity_th=0., hard_intensity_th=True,
                                       ignore_region_ids=False, score_metric='linear',
                                       local_size=5, w_ctdist=2, w_lcdist=1, w_int=1, w_nbdist=2,
                                       ignore_nan=True, nan_mask=0., inf_mask=-1000.,
                                       update_chrom_coords=False, chrom_share_spots=False,
                                       distance_zxy=_distance_zxy, distance_limits=[200,3000],
                                       return_indices=False, verbose=True):
    """picking.py:902-1200 — pick one spot per region and chromosome by dynamic programming over the regions in id order:
    the spot scores (E-step, against references made from ``sel_spot_list``, by default the naive picks) plus the
    neighbour-distance scores between consecutive regions, all chromosomes of the cell optimised together.
    Outputs: _sel_spot_list, and with ``return_indices`` _sel_ind_list (indices into the merged spots of each region)."""
    return population_dynamic_pick_spots([(cell_cand_spots, region_ids, chrom_coords, sel_spot_list, ref_spot_list)], ref_spot_ids,
                                         ref_dist_metric, nb_dist_list, spot_num_th, intensity_th, hard_intensity_th, ignore_region_ids,
                                         score_metric, local_size, w_ctdist, w_lcdist, w_int, w_nbdist, ignore_nan, nan_mask, inf_mask,
                                         update_chrom_coords, chrom_share_spots, distance_zxy, distance_limits, return_indices, verbose)[0]


def _drop_dim_candidates(cell_cand_spots, intensity_th):
    """The EM's first filter (:1284-1287), which writes into the caller's lists: every non-empty table keeps its spots
    of intensity >= min(intensity_th, its brightest).  Returns the position of the last region (None without regions):
    the value the reference's loop variable is left with."""
    last = None
    for last, lists in enumerate(cell_cand_spots):
        for c, spots in enumerate(lists):
            if len(spots) > 0:
                h = np.array(spots)[:, 0]
                lists[c] = spots[h >= min(intensity_th, max(h))]
    return last


def _changed_share(new_ind_list, old_ind_list):
    """The share of picked indices that differ from the previous iteration's (:1402-1411); all of a chromosome's count
    as changed when it had none before."""
    changed = total = 0
    for new, old in zip(new_ind_list, old_ind_list):
        if len(old) == 0:
            changed += len(new)
        else:
            changed += int(np.count_nonzero(np.array(new, dtype=int) - np.array(old, dtype=int)))
        total += len(new)
    return changed / total


def population_EM_pick_spots(cells, ref_spot_ids=None, ref_dist_metric='median', nb_dist_list=None, spot_num_th=100,
                             num_iters=10, terminate_th=0.0025, intensity_th=0., hard_intensity_th=True, score_metric='linear',
                             local_size=5, w_ctdist=2, w_lcdist=1, w_int=1, w_nbdist=2,
                             distance_limits=[0, 3000], ignore_nan=True, nan_mask=0., inf_mask=-1000., update_chrom_coords=False,
                             chrom_share_spots=False, distance_zxy=_distance_zxy,
                             check_spots=True, check_th=-2., check_percentile=10., hard_dist_th=8000,
                             make_plot=False, return_indices=False, return_sel_scores=False, return_other_scores=False,
                             verbose=True, timings=None):
    """NOT a reference name.  ``EM_pick_spots_for_chromosomes`` of every cell: the candidates go up once, the merged lists
    stay on the device, and every iteration runs the cells that have not yet converged in one E-step and one forward pass.
    A cell is ``(cell_cand_spots, region_ids, chrom_coords)`` and may go on with ``sel_spot_list`` and ``ref_spot_list``.
    Returns a list with, per cell, what the reference returns for it.  ``timings``: a dict that receives the seconds of
    the upload and merge, of every iteration (and, summed over them, of the host's bookkeeping before and after, the E-step
    and the forward pass) and of the final check."""
    from . import checking
    if make_plot:
        raise NotImplementedError("make_plot=True is not built: this package draws nothing")
    cells = [list(_c) + [None] * (5 - len(_c)) for _c in cells]
    for _c in cells:
        _c[1] = np.array(_c[1], dtype=int)
        if len(_c[0]) != len(_c[1]):
            raise ValueError(f"Length of cell_cand_spots should match region_ids, while {len(_c[0])} and {len(_c[1])} received!")
    if verbose:
        print(f"-- filtering spots by intensity threshold={intensity_th}.")
    _last_i = [_drop_dim_candidates(_c[0], intensity_th) for _c in cells]
    nums = []
    for _cand, _ids, _coords in [_c[:3] for _c in cells]:
        nums.append(len(_coords) if _coords is not None else len(_cand[0]))
    for _n, _c in zip(nums, cells):
        if _n > 6 and num_iters > 0 and 1 >= terminate_th:
            # :1362-1378 hands ONE chromosome's coordinate and all the chromosomes' lists to the dynamic picker
            if _c[2] is None:
                raise TypeError("'NoneType' object is not subscriptable")
            if any(len(_s) == 0 for _spot_list in _c[0] for _s in _spot_list[1:]):
                raise IndexError("list index out of range")
            raise NotImplementedError("%d chromosomes in a cell: the reference optimises each by itself with all the chromosomes' "
                                      "candidates (:1362-1378), which is not built" % _n)
    _check_cells(cells)
    P = _dynamic_params(ref_dist_metric, spot_num_th, intensity_th, score_metric, local_size, w_ctdist, w_lcdist, w_int, w_nbdist,
                        ignore_nan, nan_mask, inf_mask, update_chrom_coords, chrom_share_spots, distance_zxy, distance_limits, verbose)
    n_out = 1 + bool(return_indices) + bool(return_sel_scores) + bool(return_other_scores)
    out = [None] * len(cells)
    live = [_k for _k, _n in enumerate(nums) if _n > 0]
    for _k, _n in enumerate(nums):
        if _n == 0:
            if verbose:
                print("-- exit for no-chromosome case.")
            out[_k] = [] if n_out == 1 else tuple([] for _a in range(n_out))
    if not live:
        return out
    _t0 = time.time()
    pop = _open_cells([cells[_k] for _k in live], distance_zxy, intensity_th, hard_intensity_th)
    if timings is not None:
        timings["upload_merge_s"] = time.time() - _t0
        timings["iterations_s"] = []
        P["timings"] = timings
    try:
        S = {}
        for _j, _k in enumerate(live):
            s = dict(sel_spot_list=cells[_k][3], ref_spot_list=cells[_k][4], check_with=_last_i[_k], iter=0, ratio=1, ratios=[], done=False)
            if s["sel_spot_list"] is None:
                if verbose:
                    print(f"-- initialize EM by naively picking spots!")
                s["sel_spot_list"], s["sel_ind_list"] = _naive_cell(pop, _j, chrom_share_spots, distance_zxy)
            else:
                s["sel_ind_list"] = [[] for _chrom_id in range(nums[_k])]
            S[_j] = s
        if num_iters == np.inf and terminate_th < 0:
            raise ValueError(f"At least one valid termination flag required!")
        local_size = int(local_size)
        P["local_size"] = local_size
        while True:
            ks = [_j for _j, s in S.items() if not s["done"] and s["iter"] < num_iters and s["ratio"] >= terminate_th]
            if not ks:
                break
            _t0 = time.time()
            got = _dynamic_cells(pop, ks, {_j: S[_j]["sel_spot_list"] for _j in ks}, {_j: S[_j]["ref_spot_list"] for _j in ks},
                                 ref_spot_ids, nb_dist_list, P)
            _step = time.time() - _t0
            if timings is not None:
                timings["iterations_s"].append(_step)
            for _j in ks:
                s = S[_j]
                s["sel_spot_list"], new = got[_j]
                s["ratio"] = _changed_share(new, s["sel_ind_list"])
                s["ratios"].append(s["ratio"])
                if verbose:
                    print(f"--- EM iter:{s['iter']}, time: {_step:.3f}, change_ratio={s['ratio']}")
                s["iter"] += 1
                s["sel_ind_list"][:len(new)] = new
                if len(new):
                    s["check_with"] = len(new) - 1
                # the share of changed picks has hovered at the threshold for five iterations (:1420)
                if len(s["ratios"]) > 5 and np.mean(s["ratios"][-5:]) <= 2 * terminate_th:
                    if verbose:
                        print("-- exit loop because of long oscillation around minimum.")
                    s["done"] = True
        _t0 = time.time()
        check_kw = dict(distance_zxy=distance_zxy, distance_limits=distance_limits, intensity_th=intensity_th,
                        ref_dist_metric=ref_dist_metric, score_metric=score_metric, local_size=local_size, w_ctdist=w_ctdist,
                        w_lcdist=w_lcdist, w_int=w_int, ignore_nan=ignore_nan, check_th=check_th, check_percentile=check_percentile,
                        hard_dist_th=hard_dist_th, return_sel_scores=True, return_other_scores=True, verbose=verbose)
        for _j, _k in enumerate(live):
            s = S[_j]
            res = [s["sel_spot_list"]] + ([s["sel_ind_list"]] if return_indices else [])
            if check_spots or return_sel_scores or return_other_scores:
                # every chromosome is checked against the indices and the coordinate of ONE chromosome, the one the
                # reference's stale loop variable names (:1430-1432): the last one, once an iteration has run
                at = s["check_with"]
                coord = None if cells[_k][2] is None else cells[_k][2][at]
                checked = [checking.check_spot_scores(_cell_merged(pop, _j), _spots, cells[_k][1], s["sel_ind_list"][at], chrom_coord=coord,
                                                      **check_kw) for _spots in s["sel_spot_list"]]
                if check_spots:
                    s["sel_spot_list"][:] = [np.array(_r[0]) for _r in checked]
                res += [[np.array(_r[1]) for _r in checked]] if return_sel_scores else []
                res += [[np.array(_r[2]) for _r in checked]] if return_other_scores else []
            out[_k] = res[0] if len(res) == 1 else tuple(res)
        if timings is not None:
            timings["check_s"] = time.time() - _t0
    finally:
        _close_cells(pop)
    return out


def EM_pick_spots_for_chromosomes(cell_cand_spots, region_ids,
                                  chrom_coords=None, sel_spot_list=None,
                                  ref_spot_list=None, ref_spot_ids=None,
                                  ref_dist_metric='median', nb_dist_list=None, spot_num_th=100,
                                  num_iters=10, terminate_th=0.0025, intensity_th=0.,
                                  hard_intensity_th=True, score_metric='linear',
                                  local_size=5, w_ctdist=2, w_lcdist=1, w_int=1, w_nbdist=2,
                                  distance_limits=[0,3000], ignore_nan=True,
                                  nan_mask=0., inf_mask=-1000., update_chrom_coords=False,
                                  chrom_share_spots=False, distance_zxy=_distance_zxy,
                                  check_spots=True, check_th=-2., check_percentile=10.,hard_dist_th=8000,
                                  make_plot=False, save_plot=False, save_path=None, save_filename='',
                                  return_indices=False, return_sel_scores=False, return_other_scores=False,
                                  verbose=True):
    """picking.py:1204-1528 — EM spot picking for the chromosomes of one cell: start from the naive picks (or
    ``sel_spot_list``), iterate ``dynamic_pick_spots_for_chromosomes`` with the last picks as references until fewer than
    ``terminate_th`` of the indices change, ``num_iters`` is reached or the change has hovered near the threshold for five
    iterations, then check the picks (``checking.check_spot_scores``).  As in the reference the first filter writes into the
    caller's ``cell_cand_spots`` and the final check reads the last chromosome's indices and coordinate for every
    chromosome.  ``make_plot=True`` is NotImplementedError."""
    if verbose:
        print(f"- EM picking spots for {len(region_ids)} regions, use chrom_coords:{(chrom_coords is not None)}")
    return population_EM_pick_spots([[cell_cand_spots, region_ids, chrom_coords, sel_spot_list, ref_spot_list]], ref_spot_ids,
                                    ref_dist_metric, nb_dist_list, spot_num_th, num_iters, terminate_th, intensity_th, hard_intensity_th,
                                    score_metric, local_size, w_ctdist, w_lcdist, w_int, w_nbdist, distance_limits, ignore_nan, nan_mask,
                                    inf_mask, update_chrom_coords, chrom_share_spots, distance_zxy, check_spots, check_th, check_percentile,
                                    hard_dist_th, make_plot, return_indices, return_sel_scores, return_other_scores, verbose)[0]


def _not_built(name, why):
    def f(*args, **kwargs):
        raise NotImplementedError("%s is not built: %s" % (name, why))
    f.__name__ = name
    f.__doc__ = "Not built: %s." % why
    return f


_LEGACY = "the single-chromosome picker is superseded by the *_for_chromosomes functions, which take one chromosome too"
dynamic_pick_spots = _not_built("dynamic_pick_spots", _LEGACY)
EM_pick_spots = _not_built("EM_pick_spots", _LEGACY)
old_spot_score_in_chromosome = _not_built("old_spot_score_in_chromosome", "spot_tools.scoring.spot_score_in_chromosome replaces it")
distance_score_in_chromosome = _not_built("distance_score_in_chromosome", "spot_tools.scoring.distance_score replaces it")
generate_distance_score_pool = _not_built("generate_distance_score_pool", "it serves the legacy single-chromosome picker only")
generate_spot_score_pool = _not_built("generate_spot_score_pool", "it serves the legacy single-chromosome picker only")
screen_RNA_based_on_refs = _not_built("screen_RNA_based_on_refs", "it works on the reference's RNA data sets, which this package does not carry")
