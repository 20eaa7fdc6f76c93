"""Domain distances of traced chromosomes on the device (reference: domain_tools/distance.py).
``_sliding_window_dist`` (:19-67) compares, at every locus, the distances inside the windows left and right of it with the
distances between the two windows; ``domain_distance`` (:69-158) does the same for two domains given by their bounds, and
``domain_pdists`` (:161-204) / ``domain_neighboring_dists`` (:231-282) call it for all pairs / for neighbours;
``_domain_contact_freq`` (:465-490) is the share of contacts in every block of a domain partition.  Here a population of
chromosome copies (or one distance map) is uploaded once (``_lib.DomainPopulation``) and each of the three is one library
call: the window statistics for every copy, locus and up to 16 window sizes, the domain distances and the
contact frequencies for a list of (copy, s1, e1, s2, e2) entries.  Finite values, infinities and zeros equal the
reference's in every bit; a NaN stands where the reference has one.

The ``population_*`` functions are the flat forms on a resident population; they are not names of the reference.  Not
built, each raising ``NotImplementedError``: the ``mean`` and ``ks`` metrics of ``domain_distance``, ``domain_stat`` /
``domain_neighboring_stats``, ``domain_correlation_pdists``, ``_local_distances``, ``_neighboring_distance``, a window size
above ``_lib.IA3_DOMAIN_MAX_WINDOW`` and more than ``_lib.IA3_DOMAIN_MAX_R`` loci.  Bounds that a Python slice would wrap
(negative ones) raise ``ValueError``; bounds past the end are clipped as a slice clips them.  There is no CPU fallback.

All ``file:line`` citations are relative to the reference tree.
"""
import numpy as np

from .. import _lib as L

_UNBUILT_METRICS = {
    'mean': "domain_distance: the 'mean' metric is not built (np.nanmean / np.nanvar over the 1e5 to 1e6 distances of a "
            "domain pair in NumPy's pairwise order is a kernel of its own)",
    'ks': "domain_distance: the 'ks' metric is not built (the statistic needs a sorted merge of the 1e5 to 1e6 distances "
          "of a domain pair, a kernel of its own)",
}


# ---- host rules ---------------------------------------------------------------------------------------------------------------

def _kind(coordinates):
    """:83-103 'matrix' for a square 2-D array (a 3 x 3 array too), 'coords' for (R, 3)."""
    shape = np.shape(coordinates)
    if len(shape) != 2:
        raise ValueError(f"Wrong input shape for coordinates, should be 2d but {len(shape)} is given")
    if shape[0] == shape[1]:
        return 'matrix'
    if shape[1] == 3:
        return 'coords'
    raise ValueError(f"Input coordinates should be distance-matrix or 3d-coordinates!")


def _dist_metric(metric):
    metric = str(metric).lower()
    if metric in _UNBUILT_METRICS:
        raise NotImplementedError(_UNBUILT_METRICS[metric])
    if metric not in L.DOMAIN_DIST_METRICS:
        raise ValueError(f"Wrong input _metric type:{metric}")
    return metric


def _starts_ends(domain_starts, R):
    """:181-184 the starts as integers and each domain's end: the next start, R for the last."""
    starts = np.array(domain_starts, dtype=int)
    ends = np.zeros(np.shape(starts))
    ends[:-1] = starts[1:]
    ends[-1] = R
    return starts, ends.astype(int)


def _pair_bounds(domain_starts, R):
    """(P, 4) bounds (s1, e1, s2, e2) of all pairs of domains in the order of scipy's pdist."""
    starts, ends = _starts_ends(domain_starts, R)
    i, j = np.triu_indices(len(starts), 1)
    return np.stack([starts[i], ends[i], starts[j], ends[j]], axis=1).astype(np.int64).reshape(-1, 4)


def _neighbor_bounds(domain_starts, R, use_local, min_dom_sz):
    """:268-275 (D - 1, 4) bounds of neighbouring domains, with ``use_local`` only the loci near their common boundary."""
    starts, ends = _starts_ends(domain_starts, R)
    s1, e1, s2, e2 = starts[:-1], ends[:-1], starts[1:], ends[1:]
    if use_local:
        ns1 = np.maximum(s1, e1 - 2 * np.maximum(e2 - s2, min_dom_sz))
        ne2 = np.minimum(e2, s2 + 2 * np.maximum(e1 - s1, min_dom_sz))
        s1, e2 = ns1, ne2
    return np.stack([s1, e1, s2, e2], axis=1).astype(np.int64).reshape(-1, 4)


def _quads(copy, bounds, R):
    """(P, 5) entries (copy, s1, e1, s2, e2) from (P, 4) bounds as the slices [s, e) take them: clipped to R, empty when
    e < s."""
    b = np.asarray(bounds, dtype=np.int64).reshape(-1, 4)
    if len(b) and b.min() < 0:
        raise ValueError("domain bounds: negative bounds (which a slice wraps) are not built")
    q = np.empty((len(b), 5), dtype=np.int64)
    q[:, 0] = copy
    for k in (0, 2):
        q[:, 1 + k] = np.minimum(b[:, k], R)
        q[:, 2 + k] = np.maximum(q[:, 1 + k], np.minimum(b[:, k + 1], R))
    return q


def _contact_starts(domain_starts, R):
    """:473-477 sorted integer starts, 0 added, R removed."""
    starts = np.sort(domain_starts).astype(int)
    if 0 not in starts:
        starts = np.concatenate([np.array([0]), starts])
    if R in starts:
        starts = np.setdiff1d(starts, [R])
    return starts


def _as_results(values, int_zero):
    """What the reference's list of ``domain_distance`` results holds: np.float64 values and Python's integer 0."""
    return [0 if z else v for v, z in zip(values, int_zero)]


def _per_copy(population, domain_starts_list):
    lst = list(domain_starts_list)
    if len(lst) != population.N:
        raise ValueError("%d lists of domain starts for a population of %d copies" % (len(lst), population.N))
    return lst


def _upload(coordinates, normalization_mat=None):
    a = np.asarray(coordinates)
    if _kind(a) == 'matrix':
        return L.DomainPopulation.upload_matrix(a, normalization_mat)
    return L.DomainPopulation.upload(a, normalization_mat)


# ---- flat forms on a resident population (not names of the reference) ----------------------------------------------------------

def population_sliding_window_dists(population, window_sizes, metric='median'):
    """Not a name of the reference.  The (N, W, R) float64 array whose row [n, w] is ``_sliding_window_dist`` of copy n's
    distance map with window size ``window_sizes[w]``: the rows ``Domain_Calling_Sliding_Window`` keeps as ``dist_list``
    (domain_tools/calling.py), for every copy in one call."""
    return population.slide(window_sizes, metric)


def _population_dists(population, bounds_list, metric, allow_minus):
    """One library call for the (P_n, 4) bounds of every copy n: a list of (float64 values, integer-0 flags) per copy."""
    metric = _dist_metric(metric)
    quads = np.concatenate([_quads(n, bounds, population.R) for n, bounds in enumerate(bounds_list)])
    if len(quads) == 0:
        return [(np.zeros(0), np.zeros(0, dtype=bool)) for _ in bounds_list]
    values, zero = population.distances(quads, metric, allow_minus)
    cuts = np.cumsum([len(b) for b in bounds_list])[:-1]
    return list(zip(np.split(values, cuts), np.split(zero, cuts)))


def population_domain_pdists(population, domain_starts_list, metric='median', allow_minus_dist=False):
    """Not a name of the reference.  ``domain_pdists`` of every copy of a resident population with its own list of domain
    starts, in one call: a list of N float64 vectors in the order of scipy's pdist (where the reference returns the integer
    0, a 0.0).  The population's normalisation map, if it holds one, is applied."""
    return [v for v, _ in _population_dists(population, [_pair_bounds(s, population.R) for s in _per_copy(population, domain_starts_list)],
                                            metric, allow_minus_dist)]


def population_domain_neighboring_dists(population, domain_starts_list, metric='median', use_local=True, min_dom_sz=5,
                                        allow_minus_dist=True):
    """Not a name of the reference.  ``domain_neighboring_dists`` of every copy of a resident population, in one call: a
    list of N float64 vectors of len(starts) - 1 values."""
    return [v for v, _ in _population_dists(population, [_neighbor_bounds(s, population.R, use_local, min_dom_sz)
                                                         for s in _per_copy(population, domain_starts_list)], metric, allow_minus_dist)]


def population_domain_contact_freq(population, domain_starts_list, contact_th=400):
    """Not a name of the reference.  ``_domain_contact_freq`` of every copy of a resident population, in one call: a list of
    N symmetric (D, D) float64 matrices."""
    R = population.R
    starts_list = [_contact_starts(s, R) for s in _per_copy(population, domain_starts_list)]
    quads = []
    for n, starts in enumerate(starts_list):
        ends = np.concatenate([starts[1:], np.array([R])])
        i, j = np.tril_indices(len(starts))              # :486-489 the block [domain i, domain j] for j <= i
        quads.append(np.stack([np.full(len(i), n), starts[i], ends[i], starts[j], ends[j]], axis=1))
    freq = population.contacts(np.concatenate(quads), contact_th)
    out, at = [], 0
    for starts in starts_list:
        i, j = np.tril_indices(len(starts))
        m = np.zeros([len(starts), len(starts)])
        m[i, j] = m[j, i] = freq[at:at + len(i)]
        at += len(i)
        out.append(m)
    return out


# ---- the reference's names ----------------------------------------------------------------------------------------------------

def _sliding_window_dist(_mat, _wd, _dist_metric='median'):
    """Function to calculate sliding-window distance across one distance-map of chromosome (:19-67); ``_mat`` is the map."""
    _mat = np.asarray(_mat, dtype=np.float64)
    if _mat.ndim != 2 or _mat.shape[0] != _mat.shape[1]:
        raise ValueError("_sliding_window_dist: a square distance map is required, got shape %s" % (_mat.shape,))
    wds = L.domain_window_sizes([_wd])
    if _dist_metric not in L.DOMAIN_WINDOW_METRICS:
        raise ValueError(f"Wrong input _dist_metric")
    if len(_mat) == 0:
        return np.zeros(0)
    with L.DomainPopulation.upload_matrix(_mat) as pop:
        return pop.slide(wds, _dist_metric)[0, 0]


def domain_distance(coordinates, _dom1_bds, _dom2_bds,
                    _metric='median', _normalization_mat=None,
                    _allow_minus_distance=True):
    """Function to measure domain distances between two zxy arrays (:69-158) for the metrics 'median', 'absolute_median'
    and 'insulation'; returns a float64, or Python's integer 0 where the reference does."""
    if not isinstance(coordinates, np.ndarray):
        coordinates = np.array(coordinates)
    _metric = _dist_metric(_metric)
    _kind(coordinates)
    R = len(coordinates)
    quads = _quads(0, [[int(_b) for _b in _dom1_bds][:2] + [int(_b) for _b in _dom2_bds][:2]], R)
    if R == 0:
        return 0
    with _upload(coordinates, _normalization_mat) as pop:
        values, zero = pop.distances(quads, _metric, _allow_minus_distance)
    return _as_results(values, zero)[0]


def _check_normalization_shape(normalization_mat, R, words):
    if normalization_mat is not None:
        if np.shape(normalization_mat) != (R, R):
            raise ValueError(words)


def domain_pdists(coordinates, domain_starts, metric='median',
                  normalization_mat=None, allow_minus_dist=False):
    """Calculate domain pair-wise distances, return a vector as the same order as scipy.spatial.distance.pdist
    (:161-204)."""
    coordinates = np.array(coordinates).copy()
    _kind(coordinates)
    R = len(coordinates)
    bounds = _pair_bounds(domain_starts, R)
    _check_normalization_shape(normalization_mat, R,
                               f"Wrong shape of normalization:{np.shape(normalization_mat)}, should be equal to {(R, R)}")
    metric = _dist_metric(metric)
    _quads(0, bounds, R)
    if len(bounds) == 0:
        return np.array([])
    with _upload(coordinates, normalization_mat) as pop:
        return np.array(_as_results(*_population_dists(pop, [bounds], metric, allow_minus_dist)[0]))


def domain_neighboring_dists(coordinates, domain_starts, metric='median',
                             use_local=True, min_dom_sz=5,
                             normalization_mat=None, allow_minus_dist=True):
    """Function to calculate neighboring domain distances for domain calling (:231-282)."""
    coordinates = np.array(coordinates).copy()
    _kind(coordinates)
    R = len(coordinates)
    bounds = _neighbor_bounds(domain_starts, R, use_local, min_dom_sz)
    _check_normalization_shape(normalization_mat, R,
                               f"Wrong shape of normalization:{np.shape(normalization_mat)}, should be equal to {R}")
    metric = _dist_metric(metric)
    _quads(0, bounds, R)
    if len(bounds) == 0:
        return np.array([])
    with _upload(coordinates, normalization_mat) as pop:
        return np.array(_as_results(*_population_dists(pop, [bounds], metric, allow_minus_dist)[0]))


def _domain_contact_freq(_coordinates, _domain_starts, _contact_th=400):
    """Function to convert spot coordinates and domain starts into domain interaction frequency matrix (:465-490); a
    square ``_coordinates`` (3 x 3 too) is a distance map."""
    _coordinates = np.array(_coordinates)
    if _coordinates.ndim != 2 or (_coordinates.shape[0] != _coordinates.shape[1] and _coordinates.shape[1] != 3):
        raise ValueError("_domain_contact_freq: a distance map or (R, 3) coordinates are required, got shape %s" % (_coordinates.shape,))
    R = len(_coordinates)
    starts = _contact_starts(_domain_starts, R)
    L.domain_quads([(0, s, R, s, R) for s in starts], 1, R)
    with _upload(_coordinates) as pop:
        return population_domain_contact_freq(pop, [starts], _contact_th)[0]


# ---- not built ----------------------------------------------------------------------------------------------------------------

def domain_stat(coordinates, _dom1_bds, _dom2_bds,
                _method='ks', _normalization_mat=None,
                _allow_minus_distance=True,
                _make_plot=False, _return_pval=True):
    raise NotImplementedError("domain_stat is not built: its results are p-values of scipy.stats.ks_2samp / ttest_ind, host "
                              "statistics of sorted samples that no kernel here restates")


def domain_neighboring_stats(coordinates, domain_starts, method='ks',
                             use_local=True, min_dom_sz=5,
                             normalization_mat=None, allow_minus_dist=True,
                             return_pval=True):
    raise NotImplementedError("domain_neighboring_stats is not built: it is a loop of domain_stat, whose p-values are not built")


def domain_correlation_pdists(coordinates, domain_starts):
    raise NotImplementedError("domain_correlation_pdists is not built: np.corrcoef / np.ma.corrcoef go through BLAS, whose "
                              "summation order is not stated, so the result cannot be restated bit for bit")


def _local_distances(_zxy, dom_sz=5):
    raise NotImplementedError("_local_distances is not built: a host loop of np.nanmean and np.linalg.norm over a few loci, "
                              "with nothing for the device to do")


def _neighboring_distance(zxys, spot_ids=None, radius=5):
    raise NotImplementedError("_neighboring_distance is not built: a host loop of np.nanmean and np.linalg.norm over a few "
                              "loci, with nothing for the device to do")
