"""The cases of the chromosomal spot scores (spot_tools/scoring.py): one small population and the calls made on it.

``population()`` is twelve chromosomes of at most 40 regions and 130 candidate spots, each chosen for what can go wrong in
csrc/score.hip; ``fixture_calls()`` lists (key, f) where ``f(ns)`` calls the functions of a namespace ``ns`` -- the
reference's module when scripts/make_scoring_golden.py writes tests/golden/scoring.npz, this package's module in the tests --
and returns a list of arrays, stored as ``<key>__<i>``.  An exception of the reference is part of its behaviour: it is
stored as the text ``<type>: <words>``."""
import numpy as np

DZXY = np.array([200., 108., 108.])
TH = 1.                                   # intensity_th of the scoring calls
LOCAL_SIZES = [1, 2, 5, 6, 33]
REF_METRICS = ['median', 'mean', 'rg', 'cdf']
SIGNATURE_NAMES = ['distance_score', 'intensity_score', '_cum_prob', '_center_distance', '_local_distance', '_neighboring_distance',
                   'neighboring_distances', '_filter_intensities', 'generate_ref_from_chromosome', 'spot_score_in_chromosome',
                   'radius_of_gyration', 'chromosomal_spot_scores', 'Normalize_Intensities', 'generate_cdf_scores',
                   'log_distance_scores', 'exp_distance_scores']
# (name, keyword arguments of chromosomal_spot_scores)
SCORE_VARIANTS = [
    ("plain", dict()),
    ("lim500", dict(distance_limits=[0, 500], local_size=6, w_ctdist=0.5, w_lcdist=2, w_nbdist=1.5, w_int=3, nan_mask=-7, inf_mask=-9)),
    ("degen", dict(distance_limits=[1e7, 2e7], local_size=1, w_ctdist=0, w_nbdist=0)),
    ("wide", dict(local_size=33, intensity_th=0.)),
    ("keepnan", dict(ignore_nan=False, local_size=6)),
]


def same(a, b):
    """Equal in every bit where neither is NaN (so -0 differs from +0, inf equals inf), NaN where the other has a NaN."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all() and (a.view(np.uint64)[~na] == b.view(np.uint64)[~nb]).all())


def _spots(rng, ids, center, spread=(2., 8., 8.)):
    """(n, 4) rows (h, z, x, y) around ``center`` (pixels), one per id; neighbouring regions lie near each other."""
    ids = np.asarray(ids)
    walk = np.cumsum(rng.normal(size=(int(ids.max() - ids.min()) + 1, 3)) * np.array([0.3, 1.5, 1.5]), axis=0)
    zxy = np.asarray(center) + walk[ids - ids.min()] + rng.normal(size=(len(ids), 3)) * np.array(spread) * 0.2
    h = np.exp(rng.normal(size=len(ids))) * 3.
    return np.concatenate([h[:, None], zxy], axis=1)


def _chrom(cand, cand_ids, sel, sel_ids, center=None):
    return dict(cand=np.asarray(cand, dtype=np.float64), cand_ids=np.asarray(cand_ids, dtype=np.int64), sel=np.asarray(sel, dtype=np.float64),
                sel_ids=np.asarray(sel_ids, dtype=np.int64), center=center)


_POP = None


def population():
    global _POP
    if _POP is not None:
        return _POP
    rng = np.random.default_rng(20240611)
    pop = []
    ctr = np.array([12., 900., 1100.])
    # 0: one candidate, one selected row
    pop.append(_chrom(_spots(rng, [3], ctr), [3], _spots(rng, [3], ctr), [3]))
    # 1: 65 candidates (one past a wavefront) in regions of 1 to 4, one selected row per region
    per = np.array([1, 2, 3, 4] * 6 + [2, 3])
    ids = np.repeat(np.arange(len(per)), per)
    assert len(ids) == 65
    order = rng.permutation(65)                                      # the rows of a region are not adjacent
    pop.append(_chrom(_spots(rng, ids, ctr)[order], ids[order], _spots(rng, np.arange(len(per)), ctr), np.arange(len(per))))
    # 2: 130 candidates in 40 regions with id gaps, tied distances (a spot repeated in a region), ids unsorted
    per = rng.integers(1, 5, size=40)
    per[:5] = [4, 4, 3, 2, 4]
    while per.sum() != 130:
        k = rng.integers(5, 40)
        per[k] = min(max(per[k] + (1 if per.sum() < 130 else -1), 1), 6)
    region = np.arange(40) + np.cumsum(rng.integers(0, 2, size=40) * rng.integers(1, 4, size=40))   # gaps of 1 to 3 ids
    ids = np.repeat(region, per)
    c = _spots(rng, ids, ctr)
    c[1] = c[0]; c[2, 1:] = c[0, 1:]; c[5, 1:] = c[4, 1:]; c[9] = c[8]      # ties inside regions of 4, 4 and 3
    order = rng.permutation(130)
    sel_ids = region[rng.random(40) < 0.8]
    pop.append(_chrom(c[order], ids[order], _spots(rng, sel_ids, ctr), sel_ids))
    # 3: ids at 0 and at the last region; region 5 has no forward region but a reverse one, region 7 the other way round
    ids = np.array([0, 0, 1, 2, 2, 2, 4, 5, 5, 7, 8, 8, 8, 8, 39, 39])
    sel_ids = np.array([0, 1, 2, 4, 5, 7, 8, 39])
    pop.append(_chrom(_spots(rng, ids, ctr), ids, _spots(rng, sel_ids, ctr), sel_ids))
    # 4: two and three selected rows with the same id
    ids = np.repeat(np.arange(12), 3)
    sel_ids = np.array([0, 1, 1, 2, 3, 3, 3, 4, 6, 6, 7, 9, 9, 9, 10, 11])
    order = rng.permutation(len(sel_ids))
    pop.append(_chrom(_spots(rng, ids, ctr), ids, _spots(rng, sel_ids, ctr)[order], sel_ids[order]))
    # 5: a selected row that is all NaN, one with a single NaN coordinate, a neighbourhood whose every row holds a NaN
    ids = np.repeat(np.arange(20), 2)
    sel_ids = np.arange(20)
    s = _spots(rng, sel_ids, ctr)
    s[3, 1:] = np.nan
    s[6, 2] = np.nan
    s[12, 1] = np.nan; s[13, 3] = np.nan; s[15, 1:] = np.nan; s[16, 2] = np.nan     # around region 14 (local_size 5)
    c = _spots(rng, ids, ctr)
    c[7, 1:] = np.nan
    c[10, 3] = np.nan
    pop.append(_chrom(c, ids, s, sel_ids))
    # 6: intensities at and below intensity_th, zero and negative, among candidates and selected rows
    ids = np.repeat(np.arange(10), 3)
    sel_ids = np.arange(10)
    c, s = _spots(rng, ids, ctr), _spots(rng, sel_ids, ctr)
    c[:8, 0] = [TH, 0., -2.5, 0.5, np.nan, TH * (1 + 2**-52), -0., 1e-300]
    s[:5, 0] = [TH, 0., -1., 0.25, np.nan]
    pop.append(_chrom(c, ids, s, sel_ids))
    # 7: every selected row is NaN and dim: all four fallbacks
    ids = np.repeat(np.arange(6), 2)
    s = _spots(rng, np.arange(6), ctr)
    s[:, 1:] = np.nan
    s[:, 0] = [0.5, 0., -1., np.nan, TH, 0.1]
    pop.append(_chrom(_spots(rng, ids, ctr), ids, s, np.arange(6)))
    # 8: selected spots that coincide (neighbour and local distances of exactly 0: ties at vmin = 0), candidates on them
    sel_ids = np.arange(9)
    s = _spots(rng, sel_ids, ctr)
    s[1:6, 1:] = s[0, 1:]
    ids = np.repeat(np.arange(9), 2)
    c = _spots(rng, ids, ctr)
    c[::2, 1:] = s[:, 1:]
    pop.append(_chrom(c, ids, s, sel_ids))
    # 9: a given centre
    ids = np.repeat(np.arange(15), rng.integers(1, 4, size=15))
    pop.append(_chrom(_spots(rng, ids, ctr), ids, _spots(rng, np.arange(15), ctr), np.arange(15), center=np.array([11.5, 903.25, 1096.])))
    # 10: a given centre with NaN rows, and selected ids that miss regions
    ids = np.repeat(np.arange(0, 30, 2), 2)
    sel_ids = np.array([0, 2, 3, 8, 10, 11, 12, 20, 28])
    s = _spots(rng, sel_ids, ctr)
    s[4, 1:] = np.nan
    pop.append(_chrom(_spots(rng, ids, ctr), ids, s, sel_ids, center=np.array([13., 880., 1120.5])))
    # 11: negative ids and a far one
    ids = np.array([-3, -3, -2, -1, -1, -1, 0, 1, 1, 2, 100000, 100000, 100001])
    sel_ids = np.array([-4, -3, -1, 0, 2, 99999, 100001])
    pop.append(_chrom(_spots(rng, np.clip(ids, -5, 20), ctr), ids, _spots(rng, np.clip(sel_ids, -5, 20), ctr), sel_ids))
    assert len(pop) == 12 and max(len(p["cand"]) for p in pop) == 130
    _POP = pop
    return pop


def zxys(spots):
    return spots[:, 1:4] * DZXY


def _guard(f):
    """The result of f(), or the text of what it raised (IndexError, TypeError and ValueError are the reference's own)."""
    try:
        out = f()
    except (ValueError, IndexError, TypeError) as e:
        return [np.array("%s: %s" % (type(e).__name__, e))]
    if isinstance(out, tuple):
        return [np.asarray(o) for o in out]
    return [np.asarray(out)]


def given_refs():
    rng = np.random.default_rng(5)
    r = [np.abs(rng.normal(size=31)) * 400., np.abs(rng.normal(size=17)) * 300., np.abs(rng.normal(size=23)) * 350., np.exp(rng.normal(size=29)) * 3.]
    r[0][3] = np.nan
    r[2][[0, 5]] = r[2][1]
    return r


def value_cases():
    """(name, function, args, kwargs) of the stand-alone score functions on crafted arrays."""
    rng = np.random.default_rng(9)
    ref = np.round(np.abs(rng.normal(size=40)) * 300.)          # ties
    ref[[2, 7, 9]] = 0.                                          # ... at vmin = 0
    ref[[4, 11]] = 500.                                          # ... and at vmax = 500
    ref[5] = np.nan
    ref[6] = np.inf
    x = np.concatenate([np.array([0., -0., -1., 500., 500.0000001, np.nan, np.inf, -np.inf, 1e9]), ref[:12], np.abs(rng.normal(size=20)) * 300.])
    x2 = x.reshape(-1, 1)
    out = []
    for lim in ([-np.inf, np.inf], [0, np.inf], [0, 500], [500, 0], [700., 700.], [1e7, 2e7], [-5, -1]):
        tag = "%g_%g" % tuple(lim)
        out.append(("cum_" + tag, "_cum_prob", (ref, x), dict(vmin=min(lim), vmax=max(lim))))
        out.append(("dcdf_" + tag, "distance_score", (x, ref), dict(metric='cdf', distance_limits=lim, weight=1.7)))
        out.append(("dlin_" + tag, "distance_score", (x, 321.5), dict(metric='linear', distance_limits=lim, weight=0.3, nan_mask=-11)))
    out.append(("cum_scalar", "_cum_prob", (ref, 250.), dict()))
    out.append(("cum_2d", "_cum_prob", (ref, x2), dict(vmin=0)))
    out.append(("cum_one", "_cum_prob", ([3.], x), dict()))
    out.append(("cum_empty", "_cum_prob", ([np.nan, np.nan], x), dict()))
    out.append(("dcdf_w0", "distance_score", (x, ref), dict(metric='cdf', weight=0)))
    out.append(("dcdf_empty", "distance_score", (x, [np.nan]), dict(metric='cdf')))
    out.append(("dcdf_upper", "distance_score", (x, ref), dict(metric='CDF', weight=2)))
    out.append(("d_other", "distance_score", (x, ref), dict(metric='ks')))
    out.append(("dlin_inf", "distance_score", (x, np.inf), dict(metric='linear')))
    inten = np.concatenate([np.array([0., -0., -3., TH, np.nan, np.inf, 1e-300]), np.exp(rng.normal(size=25)) * 3.])
    iref = np.exp(rng.normal(size=33)) * 3.
    iref[[1, 2]] = TH
    iref[3] = np.nan
    for w in (1., 0., 2.5):
        out.append(("ilin_%g" % w, "intensity_score", (inten, 2.75), dict(metric='linear', weight=w)))
        out.append(("icdf_%g" % w, "intensity_score", (inten, iref), dict(metric='cdf', weight=w, intensity_th=TH, nan_mask=-3., inf_mask=-5.)))
    out.append(("icdf_float", "intensity_score", (inten, 2.75), dict(metric='cdf')))
    out.append(("icdf_empty", "intensity_score", (inten, [np.nan]), dict(metric='cdf')))
    out.append(("i_other", "intensity_score", (inten, iref), dict(metric='CDF')))
    out.append(("ilin_default", "intensity_score", (inten, 0.), dict()))
    return out


def host_cases():
    rng = np.random.default_rng(13)
    spots = population()[6]["cand"]
    z = zxys(population()[5]["sel"])
    v = np.abs(rng.normal(size=12)) * 1500.
    return [("filter", "_filter_intensities", (spots,), dict(intensity_th=TH)),
            ("filter_default", "_filter_intensities", (spots.tolist(),), dict()),
            ("filter_mark", "_filter_intensities", (spots,), dict(intensity_th=2., invalid_dist=-1.)),
            ("rg", "radius_of_gyration", (z,), dict()),
            ("rg_clean", "radius_of_gyration", (zxys(population()[2]["cand"]),), dict()),
            ("logd", "log_distance_scores", (v,), dict()),
            ("logd_ref", "log_distance_scores", (v.tolist(),), dict(ref_length=750)),
            ("expd", "exp_distance_scores", (v,), dict()),
            ("expd_ref", "exp_distance_scores", (v,), dict(ref_length=333.))]


def geometry_calls(c):
    """The distance functions on chromosome c: (key, f)."""
    p = population()[c]
    cz, sz = zxys(p["cand"]), zxys(p["sel"])
    ctr = None if p["center"] is None else p["center"] * DZXY
    calls = [("geo%d_ct" % c, lambda ns: _guard(lambda: ns._center_distance(cz, ctr))),
             ("geo%d_nb" % c, lambda ns: _guard(lambda: ns.neighboring_distances(cz, p["cand_ids"]))),
             ("geo%d_fw" % c, lambda ns: _guard(lambda: ns._neighboring_distance(sz, p["sel_ids"]))),
             ("geo%d_nblist" % c, lambda ns: _guard(lambda: ns.neighboring_distances(cz, p["cand_ids"], use_median=False))),
             ("geo%d_fwlist" % c, lambda ns: _guard(lambda: ns._neighboring_distance(cz, p["cand_ids"], neighbor_step=2, invalid_dist=-1., use_median=False))),
             ("geo%d_nb2" % c, lambda ns: _guard(lambda: ns.neighboring_distances(cz, p["cand_ids"], neighbor_step=-2, invalid_dist=-1.)))]
    for ls in LOCAL_SIZES:
        calls.append(("geo%d_lc%d" % (c, ls), lambda ns, ls=ls: _guard(lambda: ns._local_distance(cz, p["cand_ids"], sz, p["sel_ids"], local_size=ls))))
    calls.append(("geo%d_lcself" % c, lambda ns: _guard(lambda: ns._local_distance(sz, p["sel_ids"], sz, p["sel_ids"], local_size=5, invalid_dist=-2.))))
    return calls


def reference_calls(c):
    p = population()[c]
    calls = []
    for metric in REF_METRICS:
        for ign in (True, False):
            calls.append(("ref%d_%s_%d" % (c, metric, ign), lambda ns, metric=metric, ign=ign: _guard(lambda: ns.generate_ref_from_chromosome(
                p["sel"], p["sel_ids"], distance_zxy=DZXY, chr_center=p["center"], intensity_th=TH, local_size=5, ref_dist_metric=metric,
                ignore_nan=ign))))
    return calls


def score_kwargs(variant):
    kw = dict(score_metric='cdf', intensity_th=TH, local_size=5, distance_limits=[0, np.inf])
    kw.update(dict(SCORE_VARIANTS)[variant])
    return kw


def score_calls(c):
    p = population()[c]
    calls = []
    for variant, _ in SCORE_VARIANTS:
        kw = score_kwargs(variant)
        calls.append(("css%d_%s" % (c, variant), lambda ns, kw=kw: _guard(lambda: ns.chromosomal_spot_scores(
            p["cand"], p["cand_ids"], p["sel"], p["sel_ids"], chr_center=p["center"], distance_zxy=DZXY, verbose=False, **kw))))
    calls.append(("css%d_sum" % c, lambda ns: _guard(lambda: ns.chromosomal_spot_scores(
        p["cand"], p["cand_ids"], p["sel"], p["sel_ids"], chr_center=p["center"], distance_zxy=DZXY, verbose=False, intensity_th=TH,
        return_separate_scores=False))))
    for metric, ref_metric in (('linear', 'median'), ('linear', 'mean'), ('cdf', 'median')):
        calls.append(("ssc%d_%s_%s" % (c, metric, ref_metric), lambda ns, metric=metric, ref_metric=ref_metric: _guard(lambda: ns.spot_score_in_chromosome(
            p["cand"], p["cand_ids"], p["sel"], p["sel_ids"], chr_center=p["center"], ref_dist_metric=ref_metric, distance_zxy=DZXY,
            distance_limits=[0, 500], metric=metric, intensity_th=TH, local_size=5, w_lcdist=0.1, nan_mask=-3., verbose=False))))
    return calls


def other_calls():
    p = population()[1]
    r = given_refs()
    calls = [("css_given_cdf", lambda ns: _guard(lambda: ns.chromosomal_spot_scores(
                 p["cand"], p["cand_ids"].tolist(), p["sel"], None, score_metric='cdf', distance_zxy=DZXY, ref_center_dists=r[0], ref_local_dists=r[1],
                 ref_neighbor_dists=r[2], ref_intensities=r[3], verbose=False))),
             ("css_given_linear", lambda ns: _guard(lambda: ns.chromosomal_spot_scores(
                 p["cand"], p["cand_ids"], p["sel"], p["sel_ids"], score_metric='linear', distance_zxy=DZXY, distance_limits=[0, 300], ref_center_dists=410.,
                 ref_local_dists=120.5, ref_neighbor_dists=222., ref_intensities=2.5, verbose=False))),
             ("css_scalar_id", lambda ns: _guard(lambda: ns.chromosomal_spot_scores(
                 p["cand"][:9], 4, p["sel"], p["sel_ids"], distance_zxy=DZXY, verbose=False))),
             ("css_linear_refs", lambda ns: _guard(lambda: ns.chromosomal_spot_scores(
                 p["cand"], p["cand_ids"], p["sel"], p["sel_ids"], score_metric='linear', distance_zxy=DZXY, verbose=False))),
             ("css_list_dzxy", lambda ns: _guard(lambda: ns.chromosomal_spot_scores(p["cand"], p["cand_ids"], p["sel"], p["sel_ids"], verbose=False))),
             ("ssc_list_dzxy", lambda ns: _guard(lambda: ns.spot_score_in_chromosome(p["cand"], p["cand_ids"], p["sel"], verbose=False))),
             ("ssc_scalar_id", lambda ns: _guard(lambda: ns.spot_score_in_chromosome(p["cand"][:9], 4, p["sel"], distance_zxy=DZXY, verbose=False))),
             ("ssc_rg", lambda ns: _guard(lambda: ns.spot_score_in_chromosome(p["cand"], p["cand_ids"], p["sel"], p["sel_ids"], ref_dist_metric='rg',
                                                                              distance_zxy=DZXY, verbose=False))),
             ("ref_list_dzxy", lambda ns: _guard(lambda: ns.generate_ref_from_chromosome(p["sel"]))),
             ("ref_other", lambda ns: _guard(lambda: ns.generate_ref_from_chromosome(p["sel"], distance_zxy=DZXY, ref_dist_metric='linear'))),
             ("ref_noids", lambda ns: _guard(lambda: ns.generate_ref_from_chromosome(p["sel"], None, DZXY, ref_dist_metric='MEAN', local_size=3))),
             ("ct_1d", lambda ns: _guard(lambda: ns._center_distance(zxys(p["cand"])[0], zxys(p["sel"])[0]))),
             ("ct_noids", lambda ns: _guard(lambda: ns.neighboring_distances(zxys(p["sel"])))),
             ("rg_1d", lambda ns: [np.array(type(ns.radius_of_gyration(np.zeros(3))).__name__)])]
    for name, fn, args, kw in value_cases() + host_cases():
        calls.append(("val_" + name, lambda ns, fn=fn, args=args, kw=kw: _guard(lambda: getattr(ns, fn)(*args, **kw))))
    return calls


def fixture_calls():
    calls = []
    for c in range(len(population())):
        calls += geometry_calls(c) + reference_calls(c) + score_calls(c)
    return calls + other_calls()
