"""Scores of candidate spots against their chromosome on the device (reference: spot_tools/scoring.py).
For every candidate spot of a traced chromosome the reference computes a centre-distance, local-distance, neighbour-distance
and intensity score against the chromosome's currently selected spots, in a Python loop per spot.  Here a population of
chromosomes is uploaded once (``_lib.ScorePopulation``) and the distances, the references and the scores of all of them are
one library call each.  ``np.log`` is taken by the host's NumPy on the downloaded arguments, one vectorised
call per score; everything before it runs on the device.  Finite values, infinities and zeros equal the reference's in
every bit; a NaN stands where the reference has one.

``population_chromosomal_spot_scores`` and ``population_score_references`` are the flat forms on a resident population;
they are not names of the reference.  The reference's names build a population of one chromosome.  Not built, each raising
``NotImplementedError``: ``generate_cdf_scores``, ``Normalize_Intensities``, more than ``_lib.IA3_SCORE_MAX_PER_REGION``
spots of one region id in a chromosome and a ``local_size`` above ``_lib.IA3_SCORE_MAX_LOCAL``.  There is no CPU fallback.

The reference's errors come before any device call, with one exception that depends on device results: a chromosome whose
reference array holds no value (``ignore_nan=False`` and nothing but NaNs) raises the reference's ValueError after the
references were computed.

All ``file:line`` citations are relative to the reference tree.
"""
import time

import numpy as np

from . import _distance_zxy
from .. import _lib as L


# ---- host steps -----------------------------------------------------------------------------------------------------------------

def _finish(val, cls, w, shape):
    """The scores from the device's values and class bytes: np.log of the arguments in one call, times the weight."""
    kind = cls & 3
    scores = np.zeros(len(val))
    scores[kind == L.SCORE_VALUE] = val[kind == L.SCORE_VALUE]
    take = kind == L.SCORE_LOG
    scores[take] = np.log(val[take]) * w
    scores[kind == L.SCORE_NEG_INF] = - np.inf
    return scores.reshape(shape)


def _no_nan(ref, words):
    ref = np.ravel(np.array(ref, dtype=np.float64))
    ref = ref[np.isnan(ref) == False]   # noqa: E712
    if len(ref) == 0:
        raise ValueError(words)
    return ref


def _rows(zxys):
    """(n, 4) rows (0, z, x, y) of (n, 3) coordinates."""
    zxys = np.asarray(zxys, dtype=np.float64)
    if zxys.ndim != 2 or zxys.shape[1] != 3:
        raise IndexError(f"Wrong shape for spot_zxys:{zxys.shape}")
    return np.concatenate([np.zeros((len(zxys), 1)), zxys], axis=1)


def _arange(n):
    return np.arange(n).astype(int)


def _reference_values(arrays, counts, scalars, metric, ignore_nan):
    """What generate_ref_from_chromosome returns for one chromosome, types included (:254-303)."""
    if metric in ('median', 'mean'):
        return tuple(np.float64(s) for s in scalars)
    kept = list(arrays)
    if metric == 'rg':
        return np.float64(scalars[0]), np.float64(scalars[1]), np.float64(scalars[2]), kept[3]
    for a, fallback in enumerate(([1000], [np.inf], [np.inf], None)):
        if counts[a] < 0 and fallback is not None:
            kept[a] = fallback
    return tuple(kept)


def _say_fallbacks(counts):
    for a, (name, end) in enumerate((("_ct_dist", '\n'), ("_lc_dist", ', '), ("_nb_dist", ', '), ("_intensities", '\n'))):
        if counts[a] < 0:
            print(f"{name} has no valid values in this chromosome", end=end)


# ---- flat forms on a resident population (not names of the reference) ----------------------------------------------------------

def population_score_references(population, intensity_th=0., local_size=5, ref_dist_metric='median', ignore_nan=True):
    """Not a name of the reference.  ``generate_ref_from_chromosome`` of every chromosome of a resident population in one
    call: a list of C tuples (_ref_center_dist, _ref_local_dist, _ref_neighbor_dist, _ref_intensities)."""
    metric = str(ref_dist_metric).lower()
    arrays, counts, scalars = population.references(metric, local_size, intensity_th, ignore_nan)
    return [_reference_values(arrays[c], counts[c], scalars[c], metric, ignore_nan) for c in range(population.C)]


def population_chromosomal_spot_scores(population, score_metric='cdf', intensity_th=1., local_size=5,
                                       w_ctdist=1, w_lcdist=1, w_int=1, w_nbdist=1, distance_limits=[0, np.inf],
                                       nan_mask=-1000, inf_mask=-1000, ignore_nan=True):
    """Not a name of the reference.  ``chromosomal_spot_scores(..., return_separate_scores=True)`` of every chromosome of
    a resident population against references made from its selected spots, in one call: a list of C tuples
    (_ct_scores, _lc_scores, _nb_scores, _int_scores)."""
    weights = [float(w_ctdist), float(w_lcdist), float(w_nbdist), float(w_int)]
    val, cls, ref_counts = population.scores(score_metric, None, local_size, intensity_th, ignore_nan, weights, distance_limits)
    for a in range(3):
        if weights[a] != 0. and (ref_counts[:, a] == 0).any():
            raise ValueError(f"Wrong input ref_dist, not enough values to calculate cdf")
    if (ref_counts[:, 3] == 0).any():
        raise ValueError(f"Wrong input data, no valid points at all.")
    scores = []
    for a in range(4):
        s = _finish(val[a], cls[a], weights[a], val[a].shape)
        if a < 3:
            if weights[a] == 0.:
                s = np.zeros(s.shape)      # :20-21 the early return, before any mask
            else:
                s[(cls[a] & L.SCORE_NAN_IN) != 0] = nan_mask
        else:
            s[np.isnan(s)] = nan_mask
            s[np.isinf(s)] = inf_mask
        scores.append(s)
    at = population.cand_start
    return [tuple(s[at[c]:at[c + 1]].copy() for s in scores) for c in range(population.C)]


# ---- the reference's names ----------------------------------------------------------------------------------------------------

def distance_score(dist, ref_dist, weight=1.,
                   metric='linear', distance_limits=[-np.inf, np.inf],
                   nan_mask=-1000, inf_mask=-1000.):
    """Function to calculate distance score given a reference number (:6-51); a zero weight gives zeros."""
    _dist = np.array(dist)
    _w = float(weight)
    metric = metric.lower()
    _scores = np.zeros(np.shape(_dist))
    if _w == 0.:
        return _scores
    if metric == 'linear':
        _ref_dist = float(ref_dist)
        if _dist.ndim == 0:
            raise TypeError("'numpy.float64' object does not support item assignment")
        val, cls, _ = L.score_values(_dist, L.IA3_SCORE_KIND_DIST_LINEAR, ref_scalar=_ref_dist, weight=_w,
                                     limit_hi=max(distance_limits))
    elif metric == 'cdf':
        _ref_dist = _no_nan(ref_dist, f"Wrong input ref_dist, not enough values to calculate cdf")
        val, cls, _ = L.score_values(np.array(dist, dtype=np.float64), L.IA3_SCORE_KIND_DIST_CDF, ref_array=_ref_dist, weight=_w,
                                     limit_lo=min(distance_limits), limit_hi=max(distance_limits))
    else:
        raise ValueError(f"metric type:{metric} has not been supported yet!")
    _scores = _finish(val, cls, _w, np.shape(_dist))
    _scores[np.isnan(_dist)] = nan_mask      # inf_mask is not used, as in the reference
    return _scores


def intensity_score(intensity, ref_intensities, weight=1.,
                    metric='linear', intensity_th=0.,
                    nan_mask=0., inf_mask=-1000.):
    """Intensity score (:53-78); a metric other than 'linear' and 'cdf' gives zeros, as in the reference."""
    _int = np.array(intensity)
    _w = float(weight)
    _scores = np.zeros(np.shape(_int))
    if metric == 'linear':
        _ref = float(ref_intensities)
        val, cls, _ = L.score_values(_int, L.IA3_SCORE_KIND_INT_LINEAR, ref_scalar=_ref, weight=_w)
        _scores = _finish(val, cls, _w, np.shape(_int))
    elif metric == 'cdf':
        if isinstance(ref_intensities, int) or isinstance(ref_intensities, float):
            raise ValueError(f"ref_intensity in {metric} mode should be an array rather than one value")
        _ref = _no_nan(ref_intensities, f"Wrong input data, no valid points at all.")
        val, cls, _ = L.score_values(_int, L.IA3_SCORE_KIND_INT_CDF, ref_array=_ref, weight=_w, limit_lo=intensity_th)
        _scores = _finish(val, cls, _w, np.shape(_int))
    _scores[np.isnan(_scores)] = nan_mask
    _scores[np.isinf(_scores)] = inf_mask
    return _scores


def _cum_prob(data, target_value, vmin=-np.inf, vmax=np.inf):
    """Function to calculate CDF from a dataset (:81-107)."""
    data = _no_nan(data, f"Wrong input data, no valid points at all.")
    target_value = np.array(target_value, dtype=np.float64)
    if len(target_value.shape) == 0:
        target_value = np.array([target_value], dtype=np.float64)
    val, _, _ = L.score_values(target_value, L.IA3_SCORE_KIND_CUM_PROB, ref_array=data, limit_lo=vmin, limit_hi=vmax)
    return val.reshape(np.shape(target_value))


def _center_distance(spot_zxys, center=None):
    """Function to calculate center distance (:109-122).  One (3,) spot is three numbers and stays on the host."""
    _zxys = np.array(spot_zxys)
    if len(_zxys.shape) == 1:
        _ref_center = np.nanmean(_zxys, axis=0) if center is None else center
        return np.linalg.norm(_zxys - _ref_center)
    if len(_zxys.shape) != 2:
        raise IndexError(f"Wrong shape for spot_zxys:{_zxys.shape}")
    rows = _rows(_zxys)
    if center is not None and np.size(center) != 3:
        raise ValueError("_center_distance: one (z, x, y) centre is required, got shape %s" % (np.shape(center),))
    if len(rows) == 0:
        return np.zeros(0)
    with L.ScorePopulation.upload([rows], None, [rows], None, None if center is None else [center], (1, 1, 1)) as pop:
        return pop.geometry()[0]


def _local_distance(spot_zxys, spot_ids, sel_zxys, sel_ids,
                    local_size=5, invalid_dist=np.nan):
    """Function to caluclate local distance (:124-155)."""
    rows = _rows(np.array(spot_zxys))
    _spot_ids = np.array(spot_ids, dtype=int)
    _sel_ids = np.array(sel_ids, dtype=int)
    L.score_half(local_size)
    if len(rows) == 0:
        return np.array([])
    if len(_sel_ids) == 0:
        return np.array([invalid_dist] * len(rows))
    with L.ScorePopulation.upload([rows], [_spot_ids], [_rows(np.array(sel_zxys))], [_sel_ids], None, (1, 1, 1)) as pop:
        return pop.geometry(local_size, 1, invalid_dist)[1]


def _neighbors(spot_zxys, spot_ids, neighbor_step, invalid_dist, use_median):
    rows = _rows(np.array(spot_zxys))
    _ids = _arange(len(rows)) if spot_ids is None else np.array(spot_ids, dtype=int)
    L.score_step(neighbor_step)
    if len(rows) == 0:
        return np.array([]), np.array([])
    with L.ScorePopulation.upload([rows], [_ids], [rows], [_ids], None, (1, 1, 1)) as pop:
        if use_median:
            geom = pop.geometry(1, neighbor_step, invalid_dist)
            return geom[2], geom[3]
        fwd, rev = pop.neighbor_lists(neighbor_step, invalid_dist)
        return fwd[0], rev[0]


def _neighboring_distance(spot_zxys, spot_ids=None,
                          neighbor_step=1, invalid_dist=np.nan,
                          use_median=True):
    """Function to calculate neighboring distances between list of spot_zxys (:157-178): the forward side."""
    return _neighbors(spot_zxys, spot_ids, neighbor_step, invalid_dist, use_median)[0]


def neighboring_distances(spot_zxys, spot_ids=None,
                          neighbor_step=1, invalid_dist=np.nan,
                          use_median=True):
    """Function to calculate neighboring distances between list of spot_zxys (:180-205): forward and reverse."""
    return _neighbors(spot_zxys, spot_ids, neighbor_step, invalid_dist, use_median)


def _filter_intensities(spots, intensity_th=0., invalid_dist=np.nan):
    """Function to filter intensities from spots (:208-214); np.array copies, the caller's spots stay as they are."""
    _spots = np.array(spots)
    _intensities = _spots[:, 0]
    _intensities[_intensities <= intensity_th] = invalid_dist
    return _intensities


def generate_ref_from_chromosome(sel_spots, sel_ids=None, distance_zxy=_distance_zxy,
                                 chr_center=None, intensity_th=0.,
                                 local_size=5, ref_dist_metric='median', ignore_nan=True):
    """Generate all reference scoring info from pre-selected chromosomes (:217-303).
    Outputs:
        _chr_center_dist, _ref_local_dist, _ref_neighbor_dist, _ref_intensities"""
    _spots = np.array(sel_spots)
    if sel_ids is None:
        _ids = _arange(len(_spots))
    else:
        if len(sel_ids) != len(sel_spots):
            raise IndexError(f"Wrong input ")
        _ids = np.array(sel_ids, dtype=int)
    distance_zxy[np.newaxis, :]                  # a list, the default included, is refused here as in the reference (:243)
    ref_dist_metric = ref_dist_metric.lower()
    L.ScorePopulation._ref_metric(ref_dist_metric)
    L.score_half(local_size)
    with L.ScorePopulation.upload([_spots], [_ids], [_spots], [_ids], None if chr_center is None else [chr_center], distance_zxy) as pop:
        arrays, counts, scalars = pop.references(ref_dist_metric, local_size, intensity_th, ignore_nan)
    _say_fallbacks(counts[0])
    return _reference_values(arrays[0], counts[0], scalars[0], ref_dist_metric, ignore_nan)


def _ids_of(ids, n, name):
    if isinstance(ids, list) or isinstance(ids, np.ndarray):
        return np.array(ids, dtype=int)
    if isinstance(ids, int) or isinstance(ids, float) or isinstance(ids, np.int32):
        return np.ones(n, dtype=int) * int(ids)
    raise TypeError(f"Wrong input type for {name}, should be either np.ndarray/list or int/np.int32")


def spot_score_in_chromosome(spots, spot_ids, sel_spots,
                             sel_ids=None, chr_center=None,
                             ref_center_dist=None, ref_local_dist=None, ref_neighbor_dist=None,
                             ref_intensities=None, ref_dist_metric='median',
                             ignore_nan=True, nan_mask=0., inf_mask=-1000.,
                             distance_zxy=_distance_zxy, distance_limits=[0,np.inf], metric='linear',
                             intensity_th=0., local_size=5, w_ctdist=1, w_lcdist=0.1, w_int=1, verbose=True):
    """Function to generate spot_scores in a given chromosomes selected spots (:306-407).
    Outputs:
        _scores: spot scores corresponding to spots, np.1d-array, same length as spots"""
    _spots = np.array(spots)
    _spots[:, 1:4] * distance_zxy[np.newaxis, :]    # :346 refuses a list, the default included
    _ids = _ids_of(spot_ids, len(_spots), "spot_ids")
    if len(_spots) != len(_ids):
        raise IndexError(f"Wrong input length of _spots and _ids, length should match!")
    _sel_spots = np.array(sel_spots)
    if sel_ids is None:
        _sel_ids = np.arange(len(sel_spots))
    else:
        if len(_sel_spots) != len(sel_ids):
            raise IndexError(f"Wrong input length of _sel_spots and sel_ids, length should match!")
        _sel_ids = np.array(sel_ids, dtype=int)
    _sel_spots[:, 1:4] * distance_zxy[np.newaxis, :]
    make_refs = ref_center_dist is None or ref_local_dist is None or ref_intensities is None
    if make_refs:
        L.ScorePopulation._ref_metric(metric if metric == 'cdf' else ref_dist_metric)
    if metric.lower() not in ('linear', 'cdf') and float(w_ctdist) != 0.:
        raise ValueError(f"metric type:{metric.lower()} has not been supported yet!")
    L.score_half(local_size)
    with L.ScorePopulation.upload([_spots], [_ids], [_sel_spots], [_sel_ids], None if chr_center is None else [chr_center], distance_zxy) as pop:
        if make_refs:
            if metric == 'cdf' and ref_dist_metric != metric:
                ref_dist_metric = metric
                print(f"-- adjusted ref_dist_metric to {metric} to match performance")
            if verbose:
                print(f"-- generate reference from selected spots.")
            ref_dist_metric = ref_dist_metric.lower()
            arrays, counts, scalars = pop.references(ref_dist_metric, local_size, intensity_th, ignore_nan)
            _say_fallbacks(counts[0])
            ref_center_dist, ref_local_dist, ref_neighbor_dist, ref_intensities = _reference_values(
                arrays[0], counts[0], scalars[0], ref_dist_metric, ignore_nan)
        geom = pop.geometry(local_size)
    _scores = distance_score(geom[0], ref_center_dist, weight=w_ctdist,
                             metric=metric, distance_limits=distance_limits,
                             nan_mask=nan_mask, inf_mask=inf_mask) \
        + distance_score(geom[1], ref_local_dist, weight=w_lcdist,
                         metric=metric, distance_limits=distance_limits,
                         nan_mask=nan_mask, inf_mask=inf_mask) \
        + intensity_score(_spots[:, 0], ref_intensities, weight=w_int,
                          metric=metric, intensity_th=intensity_th,
                          nan_mask=nan_mask, inf_mask=inf_mask)
    return _scores


def radius_of_gyration(zxys):
    """Function to calculate radius of gyration (:411-420); a wrong shape RETURNS the IndexError, as the reference does."""
    zxys = np.array(zxys)
    if len(np.shape(zxys)) != 2:
        return IndexError(f"zxys should be 2d-array!")
    _rs = np.linalg.norm(zxys - np.nanmean(zxys, axis=0), axis=1)
    return np.sqrt(np.nanmean(_rs**2))


def chromosomal_spot_scores(spots, region_ids,
                            sel_spots, sel_ids=None, score_metric='cdf',
                            intensity_th=1., local_size=5,
                            w_ctdist=1, w_lcdist=1, w_int=1, w_nbdist=1,
                            chr_center=None,
                            distance_zxy=_distance_zxy, distance_limits=[0,np.inf],
                            ref_center_dists=None, ref_local_dists=None,
                            ref_neighbor_dists=None, ref_intensities=None,
                            nan_mask=-1000, inf_mask=-1000, ignore_nan=True,
                            return_separate_scores=True, verbose=True):
    """NEW function to calculate chromosomal spot scores used for EM spot picking (:423-518)."""
    _spots = np.array(spots)
    if len(np.shape(_spots)) != 2:
        raise IndexError(f"Wrong shape of _spots, should be 2d array!")
    _region_ids = _ids_of(region_ids, len(_spots), "region_ids")
    _sel_spots = np.array(sel_spots)
    if len(np.shape(_sel_spots)) != 2:
        raise IndexError(f"Wrong shape of _sel_spots, should be 2d array!")
    if sel_ids is None:
        _sel_ids = np.arange(len(_sel_spots))
    else:
        _sel_ids = np.array(sel_ids)
    make_refs = ref_center_dists is None or ref_local_dists is None \
        or ref_neighbor_dists is None or ref_intensities is None
    if make_refs:
        if len(_sel_ids) != len(_sel_spots):
            raise IndexError(f"Wrong input ")
        distance_zxy[np.newaxis, :]                # generate_ref_from_chromosome refuses a list, the default included (:243)
        L.ScorePopulation._ref_metric(score_metric)
    L.score_half(local_size)
    with L.ScorePopulation.upload([_spots], [_region_ids], [_sel_spots], [_sel_ids], None if chr_center is None else [chr_center],
                                  distance_zxy) as pop:
        if make_refs:
            if verbose:
                _ref_time = time.time()
                print(f"-- generate spot score reference from sel_spots in", end=' ')
            ref_metric = score_metric.lower()
            arrays, counts, scalars = pop.references(ref_metric, local_size, intensity_th, ignore_nan)
            _say_fallbacks(counts[0])
            ref_center_dists, ref_local_dists, ref_neighbor_dists, ref_intensities = _reference_values(
                arrays[0], counts[0], scalars[0], ref_metric, ignore_nan)
            if verbose:
                print(f"in {time.time()-_ref_time:.2f}s.")
        elif verbose:
            print(f"-- use given spot score reference.")
        if verbose:
            _score_time = time.time()
            print(f"-- calculate {len(_spots)} spot scores in", end=' ')
        geom = pop.geometry(local_size)
    _ct_scores = distance_score(geom[0], ref_center_dists, weight=w_ctdist,
                                metric=score_metric, distance_limits=distance_limits,
                                nan_mask=nan_mask, inf_mask=inf_mask)
    _lc_scores = distance_score(geom[1], ref_local_dists, weight=w_lcdist,
                                metric=score_metric, distance_limits=distance_limits,
                                nan_mask=nan_mask, inf_mask=inf_mask)
    _nb_scores = distance_score(geom[4], ref_neighbor_dists, weight=w_nbdist,
                                metric=score_metric, distance_limits=distance_limits,
                                nan_mask=nan_mask, inf_mask=inf_mask)
    _int_scores = intensity_score(_spots[:, 0], ref_intensities, weight=w_int,
                                  metric=score_metric, intensity_th=intensity_th,
                                  nan_mask=nan_mask, inf_mask=inf_mask)
    _scores = _ct_scores + _lc_scores + _nb_scores + _int_scores
    if verbose:
        print(f"in {time.time()-_score_time:.2f}s.")
    if return_separate_scores:
        return _ct_scores, _lc_scores, _nb_scores, _int_scores
    else:
        return _scores


def log_distance_scores(values, ref_length=2000):
    return np.log(np.array(values) / ref_length + 1)


def exp_distance_scores(values, ref_length=2000):
    return - np.exp(np.array(values) / ref_length)


# ---- not built ----------------------------------------------------------------------------------------------------------------

def Normalize_Intensities(spots, all_spots, method='median'):
    raise NotImplementedError("Normalize_Intensities is not built: it works on the reference's spot classes (to_intensities), "
                              "which this package does not carry for picked spots")


def generate_cdf_scores(values, pos_refs, neg_refs=None):
    raise NotImplementedError("generate_cdf_scores is not built: it is scipy.stats.percentileofscore per value, used only by "
                              "classes.decode, which is not here")
