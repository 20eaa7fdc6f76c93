"""Inputs of the fitter's option tests (tests/test_fit_options_cpu.py, tests/test_gpu_fit_options.py): the case table
and the gate that admits a case, checked against the reference (oracle/np_oracle.py) and the host build of the LM core
(tests/native/lm_cpu.cpp) alone.  No GPU result enters anything in this file.

A case is a field (a stack made by tests/test_gpu_fit_pair.py::make_stack with per-spot widths, and integer seeds), a
dtype and the options handed to ``iter_fit_seed_points``.  The gate:

(a) the host LM core on every first-fit voxel set of the case (the oracle's ``gparms``) agrees with the oracle's
    first-fit row to GATE_A = 1e-5 relative in columns 0-7, a tenth of the GPU bar;
(b) float32 cases: the oracle on the stack multiplied voxelwise by 1 + 1e-6 N(0, 1) moves the rows by at most GATE_B_REL
    = 2e-5 relative in columns 0-7 and GATE_B_ABS = 2e-4 absolute in columns 8-9, with the same ``n_iter``;
(c) the oracle's rows under ``voronoi="ckdtree"`` and ``"lowest_index"`` are identical and no ball voxel is equally far
    from its seed and another one;
(d) no row of the oracle, first fit or final, has its three widths within GATE_D = 1e-3 relative of each other: an
    isotropic fit leaves the two angle columns undetermined (on the first table of this file the device and the oracle
    agreed on columns 0-7 of such a fit to the last bit and returned sines of +1 and -1).

A case that fails is replaced by another input, never given a wider bar.  ``rejected_inputs()`` holds two ill-conditioned
inputs that gate (a) must refuse (a bound-pressed narrow spot seen from two voxels off: 1.19e-4; a spot wider than its
ball: 7.78e-4).

Worst values over the table, as tests/test_fit_options_cpu.py prints them: gate (a) 7.8e-08 (w_0.5_4_3.5-iso-u16), every
other case 0; gate (b) 7.46e-06 relative (radius3-iso-f32) and 1.12e-04 absolute (sweeps_10-dense-f32); gate (d) 6.79e-03
(sweeps_10-dense-f32).  Inputs that were replaced: wide spots at radius 2 ((a) 2.7e-5, (b) 8.4e-4), seeds up to five
voxels off under deltas of 0.25 / 0.5 ((b) 1.05e-4), a spot of width 0.42 under min_w = 1.0 ((b) 2.2e-5), spots of widths
0.8 and 3.2 under (1.7, 1.9) ((a) 3e-4), a cluster on a cubic arrangement of integer seeds (95 exact ties), and a field
whose fits were isotropic under (1.7, 1.9) (gate (d)).
"""
import functools

import numpy as np

SHAPE = (24, 64, 64)
BIG_SHAPE = (24, 128, 128)
DEFAULTS = dict(radius_fit=5, min_delta_center=1.0, max_delta_center=2.5, n_max_iter=10, max_dist_th=0.1,
                min_w=0.5, max_w=4, init_w=1.5)
GATE_A = 1e-5
GATE_B_REL = 2e-5
GATE_B_ABS = 2e-4
GATE_D = 1e-3


# ---- fields ------------------------------------------------------------------------------------------------------------
def _iso():
    """eight spots at least 13 voxels apart; widths per spot: narrower than 1.0, wider than 2.0, one below the default
    min_w; seeds off their spots by up to three voxels, so that centre bounds of 1.0 and 2.5 are active"""
    spots = np.array([[6.3, 10.2, 9.6], [7.1, 30.4, 11.2], [6.6, 50.7, 10.1], [12.4, 20.3, 31.8],
                      [17.2, 12.9, 52.3], [16.8, 33.5, 50.6], [17.5, 52.2, 51.4], [11.7, 44.1, 30.9]])
    widths = np.array([[0.8, 0.85, 0.9], [1.2, 1.6, 1.7], [2.3, 2.6, 2.5], [1.0, 1.3, 1.2],
                       [0.42, 0.6, 0.65], [1.3, 1.9, 1.5], [1.1, 1.4, 2.2], [1.5, 1.2, 1.3]])
    shifts = np.array([[0, 0, 0], [0, 1, 0], [0, 0, 0], [0, 3, 0], [0, 0, 0], [0, 1, -1], [1, 0, 0], [0, -2, 1]])
    return dict(spots=spots, widths=widths, shifts=shifts, seed=7, shape=SHAPE)


def _mild():
    """the spots of _iso, every seed on its spot's voxel, no width below the default min_w: one spot narrower than 1.0,
    one wider than 2.0"""
    f = _iso()
    f["widths"] = np.array([[0.85, 1.3, 0.9], [1.2, 1.6, 1.7], [1.6, 2.4, 2.3], [1.0, 1.3, 1.2],
                            [0.7, 0.9, 1.4], [1.3, 1.9, 1.5], [1.1, 1.4, 2.2], [1.5, 1.2, 1.3]])
    f["shifts"] = np.zeros((8, 3), dtype=int)
    return f


def _aniso():
    """every spot has one width a little below 1.7 and one a little above 1.9: width bounds of (1.7, 1.9) pin two widths
    of every fit at opposite bounds, so no fit is isotropic (gate (d)).  (Widths far outside the band, 0.8 and 3.2, fail
    gate (a) at 3e-4.)"""
    f = _iso()
    f["widths"] = np.array([[1.55, 1.8, 2.05], [2.05, 1.55, 1.8], [1.55, 2.05, 1.75], [1.85, 2.05, 1.55],
                            [1.55, 1.8, 2.05], [2.05, 1.85, 1.55], [1.55, 2.05, 1.8], [1.8, 1.55, 2.05]])
    f["shifts"] = np.zeros((8, 3), dtype=int)
    return f


def _narrow():
    """spots narrow enough for the 30 voxels of a ball of radius 2 to hold their flanks and some background"""
    f = _iso()
    f["widths"] = np.array([[0.6, 0.7, 0.75], [0.7, 0.8, 0.6], [0.55, 0.65, 0.7], [0.8, 0.6, 0.7],
                            [0.65, 0.75, 0.8], [0.7, 0.9, 0.6], [0.75, 0.6, 0.85], [0.6, 0.8, 0.7]])
    f["shifts"] = np.zeros((8, 3), dtype=int)
    return f


# The cluster: a chain of four seeds A-B-C-D.  Two integer seeds whose coordinate sums differ in parity are an odd squared
# distance apart, and then no voxel is equally far from both; A and C, B and D (same parity) are more than 2 * 5 apart, so
# their balls never meet in a tie either.
_CLUSTER = np.array([[16.2, 40.9, 48.3], [16.9, 44.6, 47.2], [17.4, 50.1, 49.6], [17.5, 54.2, 48.4]])
_CLUSTER_W = np.array([[1.3, 1.9, 1.6], [1.2, 2.0, 1.8], [1.4, 1.9, 1.5], [1.3, 1.8, 1.4]])


def _clu():
    """four isolated spots and an overlapping cluster of four: the sweeps of the cluster depend on each other"""
    spots = np.concatenate([[[6.3, 10.2, 9.6], [7.1, 30.4, 11.2], [6.6, 50.7, 10.1], [12.4, 20.3, 31.8]], _CLUSTER])
    widths = np.concatenate([[[0.8, 0.85, 0.9], [1.2, 1.6, 1.7], [2.3, 2.6, 2.5], [1.0, 1.3, 1.2]], _CLUSTER_W])
    return dict(spots=spots, widths=widths, shifts=np.zeros((8, 3), dtype=int), seed=11, shape=SHAPE)


def _big():
    """the overlapping cluster of four and 77 isolated spots on a 13-voxel grid (a 9 x 9 grid without the 2 x 2 block the
    cluster sits in): after the first pair of sweeps only the cluster is left"""
    rng = np.random.RandomState(3)
    spots, widths = list(_CLUSTER + np.array([-4.0, 21.0, 19.0])), list(_CLUSTER_W)
    for i in range(9):
        for j in range(9):
            if i in (4, 5) and j in (4, 5):
                continue
            spots.append([11.0 + rng.uniform(0.1, 0.9), 8 + 13 * i + rng.uniform(0.1, 0.9), 8 + 13 * j + rng.uniform(0.1, 0.9)])
            widths.append([rng.uniform(0.9, 1.6), rng.uniform(1.1, 2.0), rng.uniform(1.1, 2.0)])
    return dict(spots=np.array(spots), widths=np.array(widths), shifts=np.zeros((len(spots), 3), dtype=int), seed=5,
                shape=BIG_SHAPE)


def _dense():
    """More than 256 seeds, so that the four of the cluster are fewer than one in 64: two planes of a staggered lattice (rows
    9 apart, 11 apart within a row, every other row shifted by 6: squared distances of 106 and more, no ball meets
    another), the cluster in the lower plane and one pair of seeds whose balls just meet (squared distance 97).  Six seeds
    have neighbours, more than one in 64, so the kernel does not keep every sweep at its first launch; the pair settles
    within the first sweeps and the cluster alone is left."""
    rng = np.random.RandomState(9)
    special = np.concatenate([_CLUSTER + np.array([-12.0, 12.0, 12.0]), [[17.3, 60.4, 60.6], [17.6, 69.3, 64.5]]])
    widths = list(_CLUSTER_W) + [[1.2, 1.4, 1.3], [1.1, 1.3, 1.4]]
    spots = list(special)
    for z in (5, 17):
        for r in range(14):
            for c in range(11):
                q = np.array([z, 5 + 9 * r, (5 if r % 2 == 0 else 11) + 11 * c], dtype=np.float64)
                if (((np.floor(special) - q) ** 2).sum(1) <= 100).any():
                    continue
                spots.append(list(q + rng.uniform(0.1, 0.9, 3)))
                widths.append([rng.uniform(0.9, 1.5), rng.uniform(1.1, 1.9), rng.uniform(1.1, 1.9)])
    return dict(spots=np.array(spots), widths=np.array(widths), shifts=np.zeros((len(spots), 3), dtype=int), seed=6,
                shape=BIG_SHAPE, dh=30.0)


_FIELDS = dict(iso=_iso, mild=_mild, aniso=_aniso, narrow=_narrow, clu=_clu, big=_big, dense=_dense)


@functools.lru_cache(maxsize=None)
def field(name):
    """(float32 stack, integer seeds (n, 3) float64) of a field; made once, do not modify"""
    from test_gpu_fit_pair import make_stack
    f = _FIELDS[name]()
    im = make_stack(f["spots"], seed=f["seed"], widths=f["widths"], shape=f["shape"], dh=f.get("dh", 300.0))
    assert im.max() < 65000.0      # no spot is clipped
    seeds = np.floor(f["spots"]) + f["shifts"]
    im = im.astype(np.float32)
    im.setflags(write=False)
    seeds.setflags(write=False)
    return im, seeds


def stack_of(case):
    im, seeds = field(case["field"])
    seeds = seeds + np.asarray(case.get("shift", (0, 0, 0)), dtype=np.float64)
    if case["dtype"] == "u16":
        im = np.round(im).astype(np.uint16)
    return im, seeds


# ---- the table ---------------------------------------------------------------------------------------------------------
def _case(name, fld, dtype="f32", shift=(0, 0, 0), legacy=False, **opt):
    return dict(name="%s-%s-%s" % (name, fld, dtype), field=fld, dtype=dtype, shift=tuple(shift), legacy=legacy, opt=opt)


def _table():
    t = []
    for dt in ("f32", "u16"):
        for r, fld in ((1, "iso"), (2, "narrow"), (3, "iso"), (4, "iso")):
            t.append(_case("radius%d" % r, fld, dt, radius_fit=r))
        t.append(_case("radius4", "clu", dt, radius_fit=4))
        t.append(_case("control", "iso", dt))
        t.append(_case("control", "clu", dt))
        for d0, d1 in ((0.25, 0.5), (2.5, 1.0), (1.5, 1.5), (4.0, 6.0)):
            t.append(_case("delta_%g_%g" % (d0, d1), "iso", dt, min_delta_center=d0, max_delta_center=d1))
        t.append(_case("delta_0.25_0.5_shifted", "mild", dt, shift=(0, 2, -1), min_delta_center=0.25, max_delta_center=0.5))
        t.append(_case("delta_2.5_1_shifted", "clu", dt, shift=(0, 1, 0), min_delta_center=2.5, max_delta_center=1.0))
        for w0, w1, wi, fld in ((1.0, 2.0, 1.5, "mild"), (0.5, 4, 3.5, "iso"), (0.2, 8.0, 0.6, "iso"), (1.7, 1.9, 1.8, "aniso")):
            t.append(_case("w_%g_%g_%g" % (w0, w1, wi), fld, dt, min_w=w0, max_w=w1, init_w=wi))
        for th in (0.0, 1e-3, 5.0, -1.0):
            t.append(_case("dist_th_%g" % th, "clu", dt, max_dist_th=th))
        for n in (-1, 0, 1, 2, 3, 5):
            t.append(_case("n_max_iter_%d" % n, "clu", dt, n_max_iter=n, max_dist_th=1e-3))
        t.append(_case("n_max_iter_-5", "clu", dt, n_max_iter=-5, max_dist_th=1e-3))
        t.append(_case("all_off", "clu", dt, radius_fit=4, min_delta_center=0.75, max_delta_center=2.0, n_max_iter=4,
                       max_dist_th=0.01, min_w=0.7, max_w=3.0, init_w=1.2))
        t.append(_case("legacy", "clu", dt, legacy=True, radius_fit=4, min_delta_center=0.75, max_delta_center=2.0,
                       n_max_iter=3, max_dist_th=0.01))
    for n in (0, 1, 3, 10):
        t.append(_case("sweeps_%d" % n, "big", "f32", n_max_iter=n, max_dist_th=1e-3))
    t.append(_case("sweeps_3", "big", "u16", n_max_iter=3, max_dist_th=1e-3))
    t.append(_case("sweeps_10", "dense", "f32", n_max_iter=10, max_dist_th=1e-3))
    t.append(_case("sweeps_4", "dense", "u16", n_max_iter=4, max_dist_th=1e-3))
    return t


CASES = _table()
SMALL = [c for c in CASES if c["field"] not in ("big", "dense")]
BIG = [c for c in CASES if c["field"] in ("big", "dense")]
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def default_of(case):
    """the same field, dtype, seeds and model at the default options"""
    return dict(case, name=case["name"] + "@defaults", opt={})


def is_control(case):
    return all(DEFAULTS[k] == v for k, v in case["opt"].items())


# ---- the reference -----------------------------------------------------------------------------------------------------
_oracle = {}


def oracle(case, voronoi="ckdtree", perturbed=False):
    """The oracle's fit of a case, made once per process and shared (do not modify): dict of ``rows`` (n, 11) float64
    after repeatfit(), ``first`` (the rows firstfit() left), ``n_iter``, ``gparms`` and ``nvox`` (their voxel counts), ``fits`` and ``nfev`` (the
    fits that ran and, where the reference records them, their function evaluations)."""
    key = (case["field"], case["dtype"], case["shift"], case["legacy"], tuple(sorted(case["opt"].items())), voronoi, perturbed)
    if key not in _oracle:
        import np_oracle as O
        im, seeds = stack_of(case)
        if perturbed:
            assert im.dtype == np.float32
            noise = np.random.RandomState(20240).standard_normal(im.shape)
            im = (im.astype(np.float64) * (1.0 + 1e-6 * noise)).astype(np.float32)
        base = O.iter_fit_seed_points_v3 if case["legacy"] else O.iter_fit_seed_points

        class Counting(base):
            fits = []

            def _gfit(self, *a):
                self.fits.append(base._gfit(self, *a))
                return self.fits[-1]

        f = Counting(im, seeds.T, **(case["opt"] if case["legacy"] else dict(case["opt"], voronoi=voronoi)))
        f.fits = []
        f.firstfit()
        first = np.array(f.ps, dtype=np.float64)
        f.repeatfit()
        _oracle[key] = dict(rows=np.array(f.ps, dtype=np.float64), first=first, n_iter=int(f.n_iter), gparms=f.gparms,
                            nvox=np.array([g[1].shape[1] for g in f.gparms], dtype=np.int32),
                            fits=sum(bool(g.success) for g in f.fits), nfev=sum(getattr(g, "nfev", 0) for g in f.fits))
    return _oracle[key]


def row_gap(a, b):
    """(largest relative difference in columns 0-7, largest absolute one in columns 8-9) of two row tables whose NaN rows
    are at the same seeds; (inf, inf) where they are not"""
    na, nb = np.isnan(a).any(axis=1), np.isnan(b).any(axis=1)
    if not np.array_equal(na, nb):
        return np.inf, np.inf
    a, b = a[~na].astype(np.float64), b[~nb].astype(np.float64)
    if len(a) == 0:
        return 0.0, 0.0
    return (float((np.abs(a[:, :8] - b[:, :8]) / np.abs(b[:, :8])).max()), float(np.abs(a[:, 8:10] - b[:, 8:10]).max()))


# ---- the gate ----------------------------------------------------------------------------------------------------------
def gate_a_fits(lm, gparms, first, kind, delta, legacy=False, **widths):
    """largest relative difference in columns 0-7 between the host LM core on the voxel sets ``gparms`` and the rows
    ``first``; inf where one side fits and the other does not"""
    from test_lm_core_cpu import cfit, cfit_v3
    worst = 0.0
    for (im_, X, center), ref in zip(gparms, first):
        if legacy:
            rc, p, x, info = cfit_v3(lm, im_, X, center, delta, kind)
        else:
            rc, p, x, info = cfit(lm, im_, X, center, delta, kind, **widths)
        if rc or np.isnan(ref).any():
            if not (rc and np.isnan(ref).all()):
                return np.inf
            continue
        rel = np.abs(p[:8].astype(np.float64) - ref[:8]) / np.abs(ref[:8])
        worst = max(worst, float(rel.max()) if np.isfinite(rel).all() else np.inf)
    return worst


def gate_a(lm, case):
    o = oracle(case)
    opt = dict(DEFAULTS, **case["opt"])
    return gate_a_fits(lm, o["gparms"], o["first"], 1 if case["dtype"] == "u16" else 0, opt["min_delta_center"],
                       legacy=case["legacy"], min_w=opt["min_w"], max_w=opt["max_w"], init_w=opt["init_w"])


def gate_b(case):
    """(relative move of columns 0-7, absolute move of columns 8-9, n_iter equal) under the 1e-6 perturbation"""
    a, b = oracle(case), oracle(case, perturbed=True)
    rel, ab = row_gap(b["rows"], a["rows"])
    return rel, ab, a["n_iter"] == b["n_iter"]


def exact_ties(case):
    """number of (seed, ball voxel) pairs in which another seed is exactly as far from the voxel as the seed itself"""
    from harness.fit_views_ref import ball_voxels
    im, seeds = stack_of(case)
    r = dict(DEFAULTS, **case["opt"])["radius_fit"]
    ties = 0
    for i, c in enumerate(seeds):
        X = ball_voxels(c, r, im.shape).T.astype(np.float64)
        mine = ((X - c) ** 2).sum(1)
        for j, d in enumerate(seeds):
            if j != i and ((c - d) ** 2).sum() <= (2.0 * r) ** 2:
                ties += int((((X - d) ** 2).sum(1) == mine).sum())
    return ties


def gate_c(case):
    """(rows of the two Voronoi rules identical, number of exact ties)"""
    if case["legacy"]:    # the legacy class has one rule (lowest index)
        return True, exact_ties(case)
    a, b = oracle(case), oracle(case, voronoi="lowest_index")
    same = a["rows"].tobytes() == b["rows"].tobytes() and a["n_iter"] == b["n_iter"]
    return same, exact_ties(case)


def gate_d(case):
    """smallest relative spread (max - min) / max of the three widths over the oracle's first-fit and final rows.  The
    angles enter the model through the differences of the inverse squared widths alone: a fit whose three widths sit at
    one bound is isotropic, its two angle columns are whatever the solver's rounding left there (the sines saturate at
    +1 or -1), and no bar on columns 8-9 can hold.  Such inputs are not admitted: the spread is at least GATE_D."""
    o = oracle(case)
    worst = np.inf
    for rows in (o["first"], o["rows"]):
        w = rows[~np.isnan(rows).any(axis=1), 5:8]
        if len(w):
            worst = min(worst, float(((w.max(axis=1) - w.min(axis=1)) / w.max(axis=1)).min()))
    return worst


# ---- negative control --------------------------------------------------------------------------------------------------
def rejected_inputs():
    """The two ill-conditioned first fits gate (a) has to refuse: (name, image, seeds, options).  A spot of width 0.7
    under min_w = 0.8 at radius 3, its seed two voxels off and delta 0.5; a spot of width 3 in a ball of radius 2."""
    from test_gpu_fit_pair import make_stack
    two = np.array([[6.3, 10.2, 9.6], [7.1, 30.4, 11.2]])
    a = make_stack(two, widths=np.array([[1.2, 1.6, 1.7], [0.7, 0.8, 0.8]])).astype(np.float32)
    spot = np.array([[12.4, 30.3, 31.8]])
    b = make_stack(spot, seed=4, widths=np.array([[3.0, 3.0, 3.0]])).astype(np.float32)
    return [("narrow_under_min_w", a, np.floor(two[1:]) + [0, 2, 0], dict(radius_fit=3, min_delta_center=0.5, min_w=0.8)),
            ("wider_than_the_ball", b, np.floor(spot), dict(radius_fit=2))]
