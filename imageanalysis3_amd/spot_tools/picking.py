"""spot_tools/picking.py — of the reference's module ``assign_spots_to_chromosomes`` (:767-794), which
``segmentation_tools.chromosome.select_candidate_chromosomes`` is built on, and the population picker (:1567-2342):
``convert_spots_to_hzxys``, ``extract_intensities``, ``pick_spots_by_intensities``, ``chromosome_center_dists``,
``local_center_dists``, ``generate_reference_from_population`` (E-step), ``cum_val``, ``slow_cum_val``,
``pick_spots_by_scores`` (M-step) and ``evaluate_differences``, run on the device by csrc/pick.hip on a
population that is uploaded once (``upload_population`` / ``_lib.PickPopulation``) and stays resident.  Every result is the
reference's bit for bit on the same host: distances in NumPy's two norm forms, ``np.nanmean`` in row order, the literal
``cum_val`` search, ``np.argmax`` / ``np.nanmax`` selection, and scores from this host's ``np.log`` (tabled per search
node).  ``em_pick_spots`` is the loop the reference's users write around these; it is not a reference name.

The per-cell pickers (``naive_pick_spots*``, ``dynamic_pick_spots*``, ``EM_pick_spots*``), ``merge_spot_list`` and
``screen_RNA_based_on_refs`` stay the reference's.

All ``file:line`` citations are relative to the reference tree.
"""
import bisect
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
