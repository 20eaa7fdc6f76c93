"""The cases of the per-cell spot pickers (spot_tools/picking.py :14-64, :662-1563 and checking.py:9): a few small cells and
the calls made on them.

A cell is ``(cell_cand_spots, region_ids, chrom_coords)``: at most 24 regions, at most 6 candidates per chromosome and
region, spots of 11 columns (h, z, x, y, ...).  Every cell is built from a seed, so a machine without the reference makes the
same inputs; a call builds its cell anew, because the EM writes into its caller's lists.  ``fixture_calls()`` lists
(key, f) where ``f(ns)`` calls the functions of a namespace ``ns`` -- the reference's modules when
scripts/make_cell_picking_golden.py writes tests/golden/cell_picking.npz, this package's in the tests -- and returns a list
of arrays, stored as ``<key>__<i>``.  An exception of the reference is part of its behaviour: it is stored as the text
``<type>: <words>``.

THE TIE RULE.  The fixture is the reference run with ``np.argsort``'s default kind pinned to 'stable' (ascending index among
equal keys, NaN last), because the default kind's order on ties depends on the host's CPU; ``flag_<key>`` says whether
the unpinned run gave the same outputs, which every 'linear' case must."""
import types

import numpy as np

DZXY = np.array([200., 108., 108.])
W = 11
TH = 1.
SIGNATURE_NAMES = ['naive_pick_spots', 'merge_spot_list', 'naive_pick_spots_for_chromosomes', 'dynamic_pick_spots_for_chromosomes',
                   'EM_pick_spots_for_chromosomes', '_optimized_score_combinations', '_all_score_combinations']
CHECKING_SIGNATURE_NAMES = ['check_spot_scores']


def same(a, b):
    """Equal in every bit where neither is NaN, NaN where the other has a NaN; integers and texts by value."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    if a.dtype.kind in 'US' or b.dtype.kind in 'US':
        return str(a) == str(b)
    if a.dtype.kind in 'iub' and b.dtype.kind in 'iub':
        return bool((a == b).all())
    a, b = a.astype(np.float64), b.astype(np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all() and (a.view(np.uint64)[~na] == b.view(np.uint64)[~nb]).all())


def flat(out):
    """The arrays of a nested result, depth first."""
    if isinstance(out, (list, tuple)):
        res = []
        for o in out:
            res += flat(o)
        return res
    return [np.asarray(out)]


def pack(tables):
    """A list of tables as two arrays: the shape of each (-1 columns for a 1-D empty one) and all their values."""
    tables = [np.asarray(t, dtype=np.float64) for t in tables]
    shapes = np.array([[len(t), t.shape[1] if t.ndim == 2 else -1] for t in tables], dtype=np.int64).reshape(-1, 2)
    return [shapes, np.concatenate([t.ravel() for t in tables]) if tables else np.zeros(0)]


def unpack(shapes, values):
    out, at = [], 0
    for n, w in shapes:
        if w < 0:
            out.append(np.zeros(0))
            continue
        out.append(values[at:at + n * w].reshape(n, w))
        at += n * w
    return out


def _empty():
    return np.zeros((0, W))


def make_cell(seed, C, R, ids=None, max_cand=4, coords=True, p_empty=0.15, empty_regions=(), dup=0.2, far=0.1, nan_at=None,
              only_one=(), counts=None):
    """A seeded cell.  Chromosome c walks from its own centre, 30 pixels from the next one; region r of chromosome c has 0 to
    ``max_cand`` candidates near the walk (none with probability ``p_empty``, none for any chromosome in ``empty_regions``,
    exactly one, for chromosome 0 only, in ``only_one``); with probability ``dup`` chromosome c + 1's list repeats a spot
    of chromosome c within 0.05 pixel; with probability ``far`` a candidate lies 40 pixels off (beyond the 3000 nm limit);
    about a third of the intensities lie below TH.  ``nan_at`` = (region, chromosome): its first candidate gets a NaN x.
    ``counts`` = {region: candidates per chromosome} fixes the numbers of a region."""
    rng = np.random.default_rng(seed)
    centers = np.array([[10. + 2 * c, 200. + 30. * c, 300. + 30. * (c % 2)] for c in range(C)])
    ids = np.arange(R) if ids is None else np.asarray(ids)
    span = int(ids.max() - ids.min()) + 1
    walks = [centers[c] + np.cumsum(rng.normal(size=(span, 3)) * np.array([0.3, 1.5, 1.5]), axis=0) for c in range(C)]
    cell = []
    for r in range(R):
        lists = []
        for c in range(C):
            n = int(rng.integers(1, max_cand + 1))
            if r in empty_regions or rng.random() < p_empty or (r in only_one and c > 0):
                n = 0
            if r in only_one and c == 0:
                n = 1
            if counts is not None and r in counts:
                n = counts[r][c]
            if n == 0:
                lists.append(_empty())
                continue
            t = np.abs(rng.normal(size=(n, W))) + 0.5
            t[:, 0] = np.exp(rng.normal(size=n)) * 2.
            t[:, 1:4] = walks[c][ids[r] - ids.min()] + rng.normal(size=(n, 3)) * np.array([0.4, 1.5, 1.5])
            for i in range(n):
                if rng.random() < far:
                    t[i, 2] += 40.
            if c > 0 and len(lists[c - 1]) and rng.random() < dup and r not in only_one:
                t[0] = lists[c - 1][-1]
                t[0, 1:4] += rng.normal(size=3) * 0.02
                t[0, 0] *= 1.1
            lists.append(t)
        cell.append(lists)
    if nan_at is not None and len(cell[nan_at[0]][nan_at[1]]):
        cell[nan_at[0]][nan_at[1]][0, 2] = np.nan
    return cell, ids, ([centers[c].copy() for c in range(C)] if coords else None)


# name -> arguments of make_cell
CELLS = {
    # two chromosomes, ids unsorted with gaps, region 4 empty for all, a NaN coordinate
    "A": dict(seed=11, C=2, R=12, ids=[5, 2, 9, 7, 14, 8, 0, 21, 3, 16, 12, 30], empty_regions=(4,), nan_at=(2, 0)),
    # id 6 twice (a gap of 0).  The order of the two regions is the argsort's tie order: the ids are arranged so that the
    # unpinned argsort of the generating host gives the pinned order, else the reference's own output would differ by host
    "Q": dict(seed=24, C=2, R=10, ids=[11, 6, 9, 4, 3, 8, 1, 0, 15, 6], p_empty=0.1),
    # three chromosomes, 24 regions, up to 6 candidates
    "B": dict(seed=12, C=3, R=24, ids=np.random.default_rng(5).permutation(24) * 2, max_cand=6, p_empty=0.1),
    "C1": dict(seed=13, C=1, R=10, p_empty=0.2),
    "D4": dict(seed=14, C=4, R=8, max_cand=3),
    "E6": dict(seed=15, C=6, R=4, max_cand=2, p_empty=0.1),
    # the first and the last region (by id) hold nothing
    "F": dict(seed=16, C=2, R=7, ids=[3, 0, 1, 2, 6, 4, 5], empty_regions=(1, 4)),
    "G1": dict(seed=17, C=2, R=3, empty_regions=(0, 2)),           # exactly one valid region
    "H0": dict(seed=18, C=2, R=3, empty_regions=(0, 1, 2)),        # no valid region at all
    "I7": dict(seed=19, C=7, R=3, max_cand=2, p_empty=0.3),
    # regions whose merged list has no more spots than chromosomes (one candidate and two placeholders) among others
    "J": dict(seed=20, C=3, R=9, only_one=(1, 2, 6), p_empty=0.0, dup=0.0),
    # without coordinates: every list has a spot, so every region has at least C merged spots
    "N": dict(seed=21, C=2, R=8, coords=False, p_empty=0.0, dup=0.0, max_cand=3),
    # without coordinates and with empty lists: a region with fewer merged spots than chromosomes
    "N1": dict(seed=22, C=2, R=6, coords=False, only_one=(2,), p_empty=0.0, dup=0.0),
    "S": dict(seed=23, C=2, R=14, ids=np.arange(14) * 3, max_cand=5, p_empty=0.05, far=0.3),
    # 64 merged spots in one region: the most that is built
    "K64": dict(seed=25, C=2, R=3, p_empty=0.0, dup=0.0, far=0.0, counts={1: (32, 32)}),
}
# one more than is built (NotImplementedError; not in the fixture)
K65 = dict(seed=25, C=2, R=3, p_empty=0.0, dup=0.0, far=0.0, counts={1: (33, 32)})
# the cells that run as one batch of the flat forms, and the EM's arguments there
BATCH = ["A", "Q", "B", "D4", "F", "G1", "N", "K64"]
BATCH_EM_KW = dict(return_indices=True, return_sel_scores=True, return_other_scores=True, num_iters=4)


def cell(name):
    return make_cell(**CELLS[name])


MERGE_VARIANTS = [("d", dict()), ("hard", dict(intensity_th=TH)), ("soft", dict(intensity_th=TH, hard_intensity_th=False)),
                  ("none", dict(intensity_th=None)), ("wide", dict(dist_th=2.5))]
NAIVE_VARIANTS = [("d", dict()), ("share", dict(chrom_share_spots=True)), ("hard", dict(intensity_th=TH)),
                  ("soft", dict(intensity_th=TH, hard_intensity_th=False))]
# the variants a cell is merged / naively picked with (all of them for cell A, the default one for a cell not named here)
MERGE_OF = {"A": ("d", "hard", "soft", "none", "wide"), "J": ("d", "hard"), "N1": ("d", "soft"), "S": ("d", "wide"),
            "N": ("d", "hard")}
NAIVE_OF = {"A": ("d", "share", "hard", "soft"), "N": ("d", "hard"), "J": ("d", "share"), "H0": ("d", "share")}
# (key, cell, keyword arguments); 'linear' unless the key says cdf
DYNAMIC_CASES = [
    ("A_d", "A", dict()), ("A_share", "A", dict(chrom_share_spots=True)), ("A_hard", "A", dict(intensity_th=TH)),
    ("A_soft", "A", dict(intensity_th=TH, hard_intensity_th=False)), ("A_nb0", "A", dict(w_nbdist=0)),
    ("A_lim", "A", dict(distance_limits=[0, 1500], w_ctdist=0.5, w_lcdist=2, w_int=3, nan_mask=-7., inf_mask=-9.)),
    ("A_sel", "A", dict(spot_num_th=5)), ("A_upd", "A", dict(update_chrom_coords=True)), ("A_mean", "A", dict(ref_dist_metric='mean')),
    ("A_cdf", "A", dict(score_metric='cdf', ref_dist_metric='cdf')),
    ("B_d", "B", dict()), ("B_sel", "B", dict(spot_num_th=20, local_size=7)), ("B_cdf", "B", dict(score_metric='cdf', ref_dist_metric='cdf')),
    ("C1_d", "C1", dict()), ("D4_d", "D4", dict()), ("D4_share", "D4", dict(chrom_share_spots=True)), ("E6_d", "E6", dict()),
    ("F_d", "F", dict()), ("G1_d", "G1", dict()), ("H0_d", "H0", dict()), ("J_d", "J", dict()), ("J_share", "J", dict(chrom_share_spots=True)),
    ("Q_d", "Q", dict()), ("Q_share", "Q", dict(chrom_share_spots=True)),
    ("K64_d", "K64", dict()), ("S_d", "S", dict()), ("S_cdf", "S", dict(score_metric='cdf', ref_dist_metric='cdf', distance_limits=[0, 2000])),
    ("N_d", "N", dict()), ("N_share", "N", dict(chrom_share_spots=True)),
    # the reference's errors
    ("N1_few", "N1", dict()), ("A_nblist", "A", dict(nb_dist_list=[np.ones(3), np.ones(3)])), ("A_listdz", "A", dict(distance_zxy=[200, 108, 108])),
]
EM_CASES = [
    ("A_d", "A", dict()), ("A_one", "A", dict(num_iters=1)), ("A_nocheck", "A", dict(check_spots=False)),
    ("A_all", "A", dict(return_indices=True, return_sel_scores=True, return_other_scores=True)),
    ("A_term", "A", dict(terminate_th=0.5, return_indices=True)), ("A_share", "A", dict(chrom_share_spots=True, return_indices=True)),
    ("A_hard", "A", dict(intensity_th=TH, return_indices=True, return_sel_scores=True)),
    ("A_cdf", "A", dict(score_metric='cdf', ref_dist_metric='cdf', return_indices=True, return_sel_scores=True, return_other_scores=True)),
    ("C1_all", "C1", dict(return_indices=True, return_sel_scores=True)), ("D4_idx", "D4", dict(return_indices=True, num_iters=3)),
    ("S_all", "S", dict(return_indices=True, return_sel_scores=True, return_other_scores=True, spot_num_th=10)),
    ("N_idx", "N", dict(return_indices=True)), ("Q_idx", "Q", dict(return_indices=True, return_sel_scores=True)), ("F_idx", "F", dict(return_indices=True, return_sel_scores=True)),
    # the reference's errors
    ("I7_err", "I7", dict()), ("A_noterm", "A", dict(num_iters=np.inf, terminate_th=-1.)), ("A_len", "A", dict(_cut_ids=True)),
]
EM_CASES += [(name + "_batch", name, BATCH_EM_KW) for name in BATCH] + [("H0_d", "H0", dict(return_indices=True)), ("E6_one", "E6", dict(num_iters=1, return_indices=True))]
LINEAR_KEYS = (["dyn_" + k for k, _, kw in DYNAMIC_CASES if kw.get("score_metric") != 'cdf'] +
               ["em_" + k for k, _, kw in EM_CASES if kw.get("score_metric") != 'cdf'])
# the dynamic cases whose merged lists, scores, pointers and indices the stand-alone check of csrc/ia3_cellpick.h replays
TRACED = ["A_d", "A_share", "A_soft", "A_nb0", "A_cdf", "B_d", "C1_d", "D4_d", "E6_d", "F_d", "G1_d", "J_d", "K64_d", "Q_d", "S_cdf", "N_d"]


def dynamic_kwargs(kw):
    out = dict(distance_zxy=DZXY, verbose=False)
    out.update(kw)
    return out


def run(f):
    """The arrays ``f()`` returns, or the text of what it raises."""
    try:
        return flat(f())
    except Exception as e:                                     # noqa: BLE001 -- the exception is the result
        return [np.array("%s: %s" % (type(e).__name__, e))]


def fixture_calls():
    calls = []

    def add(key, f):
        calls.append((key, lambda ns, f=f: run(lambda: f(ns))))

    for name in CELLS:
        if name == "I7":                                         # seven chromosomes: beyond what is built, the EM's error only
            continue
        for vname, kw in MERGE_VARIANTS:
            if vname not in MERGE_OF.get(name, ("d",)):
                continue

            def f(ns, name=name, kw=kw):
                cand, ids, coords = cell(name)
                return pack([ns.picking.merge_spot_list(lists, append_nan_spots=coords is not None, chrom_coords=coords, **kw) for lists in cand])
            add("merge_%s_%s" % (name, vname), f)
        if name in ("A", "J"):
            def f(ns, name=name):
                cand, ids, coords = cell(name)
                return pack([ns.picking.merge_spot_list(lists, intensity_th=TH) for lists in cand])
            add("merge_%s_plain" % name, f)
        for vname, kw in NAIVE_VARIANTS:
            if vname not in NAIVE_OF.get(name, ("d",)):
                continue

            def f(ns, name=name, kw=kw):
                cand, ids, coords = cell(name)
                return ns.picking.naive_pick_spots_for_chromosomes(cand, ids, coords, distance_zxy=DZXY, return_indices=True, verbose=False, **kw)
            add("naive_%s_%s" % (name, vname), f)
    add("merge_err_nocoords", lambda ns: ns.picking.merge_spot_list(cell("A")[0][0], append_nan_spots=True))
    add("naive_A_listdz", lambda ns: ns.picking.naive_pick_spots_for_chromosomes(*cell("A"), verbose=False))
    add("naive_A_spots_only", lambda ns: ns.picking.naive_pick_spots_for_chromosomes(*cell("A"), distance_zxy=DZXY, verbose=False))
    add("nps_A_1", lambda ns: ns.picking.naive_pick_spots(cell("A")[0], cell("A")[1], chrom_id=1, return_indices=True))
    add("nps_A_0", lambda ns: ns.picking.naive_pick_spots(cell("A")[0], cell("A")[1], chrom_id=np.int64(0)))
    add("nps_A_flat", lambda ns: ns.picking.naive_pick_spots([lists[0] for lists in cell("A")[0]], cell("A")[1], use_chrom_coord=False, return_indices=True))
    add("nps_err_len", lambda ns: ns.picking.naive_pick_spots(cell("A")[0], cell("A")[1][:3], chrom_id=0))
    add("nps_err_id", lambda ns: ns.picking.naive_pick_spots(cell("A")[0], cell("A")[1]))
    add("nps_err_chrom", lambda ns: ns.picking.naive_pick_spots(cell("C1")[0], cell("C1")[1], chrom_id=1))
    for key, name, kw in DYNAMIC_CASES:
        def f(ns, name=name, kw=kw):
            cand, ids, coords = cell(name)
            return ns.picking.dynamic_pick_spots_for_chromosomes(cand, ids, coords, return_indices=True, **dynamic_kwargs(kw))
        add("dyn_" + key, f)

    def f(ns):                                                   # the spots alone, and given selected spots as references
        cand, ids, coords = cell("B")
        sel = ns.picking.naive_pick_spots_for_chromosomes(cand, ids, coords, distance_zxy=DZXY, verbose=False)
        return ns.picking.dynamic_pick_spots_for_chromosomes(cand, ids, coords, sel_spot_list=sel, spot_num_th=20, distance_zxy=DZXY, verbose=False)
    add("dyn_B_given", f)
    for key, name, kw in EM_CASES:
        def f(ns, name=name, kw=kw):
            cand, ids, coords = cell(name)
            kw = dict(kw)
            if kw.pop("_cut_ids", False):
                ids = ids[:-1]
            return ns.picking.EM_pick_spots_for_chromosomes(cand, ids, coords, distance_zxy=DZXY, verbose=False, **kw)
        add("em_" + key, f)

    def f(ns):                                                   # :1287 writes into the caller's lists
        cand, ids, coords = cell("A")
        ns.picking.EM_pick_spots_for_chromosomes(cand, ids, coords, distance_zxy=DZXY, verbose=False, intensity_th=TH, num_iters=1)
        return pack([lists[c] for lists in cand for c in range(2)])
    add("em_A_writes", f)

    def f(ns):
        cand, ids, coords = cell("S")
        merged = [ns.picking.merge_spot_list(lists, append_nan_spots=True, chrom_coords=coords) for lists in cand]
        sel, inds = ns.picking.naive_pick_spots_for_chromosomes(cand, ids, coords, distance_zxy=DZXY, return_indices=True, verbose=False)
        a = ns.checking.check_spot_scores(merged, sel[0], ids, inds[0], chrom_coord=coords[0], distance_zxy=DZXY, return_sel_scores=True,
                                          return_other_scores=True)
        b = ns.checking.check_spot_scores(merged, sel[1], ids, None, distance_zxy=DZXY, spot_num_th=5, check_percentile=0., check_th=-1.,
                                          hard_dist_th=None, score_metric='cdf', ref_dist_metric='cdf')
        return [a, b]
    add("check_S", f)
    add("check_err_len", lambda ns: ns.checking.check_spot_scores([np.ones((2, W))], np.ones((2, W)), [1, 2, 3], distance_zxy=DZXY))
    add("check_err_type", lambda ns: ns.checking.check_spot_scores((np.ones((2, W)),), np.ones((2, W)), distance_zxy=DZXY))
    for i, (scores, share) in enumerate(combination_cases()):
        add("comb_all_%d" % i, lambda ns, s=scores, sh=share: np.array(ns.picking._all_score_combinations(s, chrom_share_spots=sh), dtype=np.int16).reshape(-1, len(s)))
        add("comb_opt_%d" % i, lambda ns, s=scores, sh=share: np.array(ns.picking._optimized_score_combinations(s, chrom_share_spots=sh), dtype=np.int16).reshape(-1, len(s)))
    add("comb_err_empty", lambda ns: ns.picking._optimized_score_combinations([]))
    add("comb_err_none", lambda ns: ns.picking._all_score_combinations([np.zeros(0)]))
    add("comb_err_few", lambda ns: ns.picking._optimized_score_combinations([np.zeros(1), np.zeros(1)]))
    return calls


def combination_cases():
    """Score lists without ties (the argsort of the combination helpers is the caller's NumPy)."""
    rng = np.random.default_rng(9)
    out = []
    for C, K in ((1, 1), (1, 4), (2, 2), (2, 5), (3, 3), (3, 7), (4, 6)):
        for share in (False, True):
            s = [rng.permutation(K).astype(np.float64) - 2. for _ in range(C)]
            if K > 4:
                s[-1][:] = -np.inf                              # a chromosome whose scores are all infinite takes all indices
            out.append((s, share))
    return out


def namespace(picking, checking):
    return types.SimpleNamespace(picking=picking, checking=checking)
