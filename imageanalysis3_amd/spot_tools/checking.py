"""spot_tools/checking.py of the reference: ``check_spot_scores`` (:9-163), the stringency check that closes
``picking.EM_pick_spots_for_chromosomes``, stated on the host over the device-backed functions of ``spot_tools.scoring``
and ``scipy.stats.scoreatpercentile``.  The scores of all the spots of ``all_spot_list`` are one call with their region ids
(the reference calls once per region; a spot's score depends on nothing but the spot, its id and the references), and the
scores that were not selected are cut out of that vector with one mask.
``filter_candidate_spots`` (:170-191) works on data frames, which this package does not carry, and is not built.

All ``file:line`` citations are relative to the reference tree.
"""
import numpy as np

from . import scoring
from . import _distance_zxy


def _unselected(n_per_region, sel_indices):
    """Mask over the spots of all regions, region after region: the scores the reference collects as 'other' (:98-107).
    Without ``sel_indices`` all of them; else, of every region that has spots and a selected index >= 0, all but that one."""
    start = np.concatenate([[0], np.cumsum(n_per_region)]).astype(int)
    mask = np.ones(start[-1], dtype=bool)
    if sel_indices is None:
        return mask
    mask[:] = False
    for k, sel in zip(range(len(n_per_region)), sel_indices):
        n = n_per_region[k]
        if n == 0 or sel < 0:
            continue
        if sel >= n:
            raise IndexError("pop index out of range")
        mask[start[k]:start[k + 1]] = True
        mask[start[k] + sel] = False
    return mask


def check_spot_scores(all_spot_list, sel_spots, region_ids=None, sel_indices=None, spot_num_th=100,
                      chrom_coord=None, distance_zxy=_distance_zxy, distance_limits=[0, np.inf],
                      intensity_th=0., ref_dist_metric='median', score_metric='linear',
                      local_size=5, w_ctdist=2, w_lcdist=1, w_int=1,
                      ignore_nan=True, nan_mask=0., inf_mask=-1000.,
                      check_th=-3.5, check_percentile=1., hard_dist_th=6000,
                      return_sel_scores=False, return_other_scores=False, verbose=False):
    """checking.py:9-163 — the selected spots with those that fail the check blanked (intensity 0, NaN elsewhere): a spot
    fails when its score (ct + lc + int of ``spot_score_in_chromosome``) lies below the threshold, when it holds a NaN, or
    when it lies farther than ``hard_dist_th`` from the mean of the selected spots.  The threshold is ``check_th`` times the
    sum of the weights, raised to the smaller of the ``check_percentile`` of the selected scores and the matching upper
    percentile of the other scores when 0 < ``check_percentile`` < 100.  References come from all spots when fewer than
    ``spot_num_th`` are selected, else from the selected ones.
    Outputs: filtered_spots, and with the flags sel_scores and other_scores."""
    from scipy.stats import scoreatpercentile
    if isinstance(all_spot_list, list):
        all_spots = np.concatenate(all_spot_list)
    elif isinstance(all_spot_list, np.ndarray):
        all_spots = all_spot_list
    else:
        raise TypeError(f"Wrong input type for all_spot_list, should be list or np.ndarray.")
    if not isinstance(sel_spots, (list, np.ndarray)):
        raise TypeError(f"Wrong input type for sel_spots, should be list or np.ndarray.")
    sel_spots = np.array(sel_spots)
    if region_ids is None:
        region_ids = np.arange(len(sel_spots))
    elif len(region_ids) != len(sel_spots):
        raise ValueError(f"Wrong input length for region_ids, not matched with sel_spots")
    else:
        region_ids = np.array(region_ids, dtype=int)
    if verbose:
        print(f"-- check spot for {len(sel_spots)} spots")
    # the regions that have an id, their sizes, and the id of every spot
    n_regions = min(len(all_spot_list), len(region_ids))
    sizes = np.array([len(all_spot_list[k]) for k in range(n_regions)], dtype=int)
    spot_ids = np.repeat(np.asarray(region_ids[:n_regions], dtype=int), sizes)
    from_all = len(sel_spots) < spot_num_th
    if verbose:
        print(f"--- use {'all' if from_all else 'selected'} spots as reference,", end=' ')
    ref_spots, ref_ids = (all_spots, spot_ids) if from_all else (sel_spots, region_ids)
    refs = scoring.generate_ref_from_chromosome(ref_spots, ref_ids, distance_zxy=distance_zxy, chr_center=chrom_coord,
                                                intensity_th=intensity_th, local_size=local_size, ref_dist_metric=ref_dist_metric,
                                                ignore_nan=ignore_nan)

    def score(spots, ids):
        return scoring.spot_score_in_chromosome(spots, ids, ref_spots, ref_ids, chrom_coord, refs[0], refs[1], refs[2], refs[3],
                                                ref_dist_metric=ref_dist_metric, ignore_nan=ignore_nan, nan_mask=nan_mask, inf_mask=inf_mask,
                                                distance_zxy=distance_zxy, distance_limits=distance_limits, metric=score_metric,
                                                intensity_th=intensity_th, local_size=local_size, w_ctdist=w_ctdist, w_lcdist=w_lcdist,
                                                w_int=w_int)
    for k in range(n_regions):
        np.array(all_spot_list[k])[:, 1:4]            # an empty region fails here, as in the reference (scoring.py:346)
    every = np.asarray(score(np.concatenate([np.array(all_spot_list[k]) for k in range(n_regions)]), spot_ids))
    sel_scores = np.array(score(sel_spots, region_ids))
    other_scores = every[_unselected(sizes, sel_indices)]
    # thresholds from the scores above the mask value
    floor = max(inf_mask, - np.inf)
    good_sel = sel_scores[sel_scores > floor]
    good_other = other_scores[other_scores > floor]
    if len(good_other) == 0:
        good_other = np.array([-np.inf])
    th_sel = scoreatpercentile(good_sel, check_percentile)
    th_other = scoreatpercentile(good_other, max(0, 100 - 100. * len(good_sel) / len(good_other) - check_percentile))
    threshold = check_th * (w_ctdist + w_lcdist + w_int)
    if verbose:
        print(f"current thresholds: {np.round([th_sel, th_other, threshold],3)}")
    if 0 < check_percentile < 100:
        threshold = max(min(th_sel, th_other), threshold)
    if verbose:
        print(f"--- applying stringency check for {len(sel_spots)} spots, threshold={threshold}")
    failed = (sel_scores < threshold) | np.isnan(sel_spots).any(axis=1)
    if hard_dist_th is not None and hard_dist_th is not False:
        failed = failed | (scoring._center_distance(sel_spots[:, 1:4] * distance_zxy, center=None) > hard_dist_th)
    filtered = sel_spots.copy()
    filtered[failed, 0] = 0
    filtered[failed, 1:] = np.nan
    if verbose:
        print(f"--- {int(failed.sum())} spots didn't pass stringent quality check.")
    out = (filtered,) + ((sel_scores,) if return_sel_scores else ()) + ((other_scores,) if return_other_scores else ())
    return out[0] if len(out) == 1 else out


def filter_candidate_spots(*args, **kwargs):
    """Not built: checking.py:170-191 filters a pandas data frame of fitted spots, which this package does not carry."""
    raise NotImplementedError("filter_candidate_spots is not built: it filters a pandas data frame of fitted spots, which this "
                              "package does not carry")
