"""Inputs of the population-picking tests (tests/test_pick_spots_cpu.py, tests/test_gpu_pick_spots.py,
scripts/make_pick_golden.py): seeded, nothing stored.

A case is a dict: ``cands[p][r]`` (``[]``, ONE 1-D row or a (k, 4) table of h, z, x, y in nm), ``ids`` (candidate and
reference ids of the regions), ``channels`` (strings, or None), ``neighbor_len``, ``center_weight``, ``local_weight``,
``split_int``, ``split_dist`` and ``centers`` (per chromosome a centre of length 3 or 4, or None).  The flow of every case:
start from the brightest candidates, one E-step, one M-step against those picks, the difference of the two picks.

Shapes are the smallest at which a rule can fail: P = 3 chromosomes, R = 9 regions, windows of 2 ids, 0-4 candidates.
The base population holds an empty region, a table with a NaN row, equal maxima of h, a repeated row (equal scores: the
first wins) and a region whose whole window is empty (NaN local centre); windows are clipped at both ends.
"""
import json

import numpy as np

CHANNELS3 = ["750", "647", "561"]
CUM_SIZES = (1, 2, 3, 4, 5, 255, 256, 257, 65537, 131073, 300001)   # 300001: the search stops at its 16th iteration


def population(seed, P, R, kmax=4, features=True, kmin=0):
    """Chromosomes as random walks of R regions (steps of ~300 nm) around centres a few um apart; per region 0..kmax
    candidates: one near the walk, the others anywhere within 1.5 um.  h on a grid of 0.25, so that equal maxima occur."""
    rs = np.random.RandomState(seed)
    cands = []
    for p in range(P):
        ctr = rs.uniform(2000, 20000, 3)
        walk = ctr + np.cumsum(rs.normal(0, 300, (R, 3)), axis=0)
        regions = []
        for r in range(R):
            k = rs.randint(kmin, kmax + 1)
            t = np.zeros((k, 4))
            for s in range(k):
                near = s == 0
                t[s, 0] = (4 if near else 1) + 0.25 * rs.randint(0, 24)
                t[s, 1:] = walk[r] + (rs.normal(0, 60, 3) if near else rs.uniform(-1500, 1500, 3))
            regions.append(t[rs.permutation(k)] if k else [])
        cands.append(regions)
    if features and P >= 3 and R >= 9:
        rows = lambda n: np.column_stack([4 + 0.25 * rs.randint(0, 24, n), rs.uniform(2000, 20000, (n, 3))])   # noqa: E731
        cands[0][2] = []                                    # an empty region
        t = rows(3)
        t[1] = np.nan                                       # a NaN row: np.argmax of h takes it
        cands[1][3] = t
        t = rows(4)
        t[3, 0] = t[1, 0] = t[:, 0].max() + 1               # equal maxima of h: the first wins
        cands[0][5] = t
        t = rows(3)
        t[2] = t[0]                                         # a repeated row: equal scores, the first wins
        cands[1][6] = t
        for r in (4, 5, 7, 8):                              # region 6 of chromosome 2: nothing picked in its window
            cands[2][r] = []
        cands[2][6] = rows(2)
        cands[0][0], cands[0][8] = rows(2), rows(3)          # the clipped windows have candidates
    return cands


def _case(cands, ids=None, channels=None, neighbor_len=2, cw=1.0, lw=1.0, split_int=False, split_dist=False, centers=None):
    R = len(cands[0])
    return dict(cands=cands, ids=list(range(R)) if ids is None else list(ids), channels=channels, neighbor_len=neighbor_len,
                center_weight=cw, local_weight=lw, split_int=split_int, split_dist=split_dist, centers=centers)


IDS_GAPS = [3, 4, 6, 7, 8, 11, 12, 13, 15]      # not 0..R-1 and not contiguous
IDS_PERM = [0, 1, 2, 5, 4, 3, 6, 7, 8]          # id order and index order of a window differ


# Entries of the case "one_d" given as ONE 1-D row.  Their values were searched (seeded) so that BOTH distances of each,
# to the chromosome centre and to the local centre, differ in the last bit between BLAS ddot's fused form and the plain
# form: a picker that lost the per-entry flag anywhere gives other bits.  scripts/make_pick_golden.py and the tests assert it.
ONE_D_ROWS = {(0, 4): [8.5, 6193.638, 15942.444, 4423.043], (2, 1): [6.0, 18274.056, 5705.08, 13700.779]}


def _one_d():
    c = population(11, 3, 9)
    for (p, r), row in ONE_D_ROWS.items():
        c[p][r] = np.array(row)                              # ONE 1-D row: BLAS norm
    c[1][4] = np.array(ONE_D_ROWS[(0, 4)]).reshape(1, 4)     # the same spot as a 1 x 4 table: plain norm
    return _case(c)


def first_row(cands, p, r):
    """Index, in population order, of the first candidate of region r of chromosome p."""
    n = 0
    for pp, regions in enumerate(cands):
        for rr, e in enumerate(regions):
            if (pp, rr) == (p, r):
                return n
            n += len(np.array(e).reshape(-1, 4)) if len(e) else 0
    raise IndexError((p, r))


def _centers(n):
    rs = np.random.RandomState(5)
    return [list(rs.uniform(2000, 20000, n)) for _ in range(3)]


CASES = {
    "base": lambda: _case(population(1, 3, 9)),
    "one_d": _one_d,
    "ids_gaps": lambda: _case(population(2, 3, 9), ids=IDS_GAPS),
    "ids_perm": lambda: _case(population(3, 3, 9), ids=IDS_PERM, neighbor_len=4),
    "centers3": lambda: _case(population(4, 3, 9), centers=_centers(3)),
    "centers4": lambda: _case(population(4, 3, 9), centers=_centers(4)),
    "split_int": lambda: _case(population(6, 3, 9, kmin=1), ids=IDS_PERM, channels=CHANNELS3 * 3, neighbor_len=4, split_int=True),
    "split_dist": lambda: _case(population(7, 3, 9, kmin=1), ids=IDS_PERM, channels=CHANNELS3 * 3, neighbor_len=4, split_dist=True),
    "split_both": lambda: _case(population(8, 3, 9, kmin=1), ids=IDS_PERM, channels=CHANNELS3 * 3, neighbor_len=4, split_int=True,
                                split_dist=True),
    "w_center0": lambda: _case(population(9, 3, 9), cw=0.0),
    "w_local0": lambda: _case(population(10, 3, 9), lw=0.0),
    # one region has no neighbour: every local distance is NaN, so only a local weight of 0 scores without IndexError
    "r1": lambda: _case(population(12, 3, 1, features=False, kmin=1), lw=0.0),
    "p1": lambda: _case(population(13, 1, 9, features=False)),
    # references longer than the 255 pivots staged in LDS, more than one workgroup
    "big": lambda: _case(population(14, 64, 300, features=False), channels=CHANNELS3 * 100, neighbor_len=7, split_int=True,
                         split_dist=True),
}
# a channel ('561') none of whose picked rows has a local centre: its reference array is empty, and a score that needs it
# is the reference's IndexError
EMPTY_REFERENCE = lambda: _case(population(7, 3, 9), ids=IDS_PERM, channels=CHANNELS3 * 3, neighbor_len=4, split_dist=True)   # noqa: E731
SMALL = [n for n in CASES if n != "big"]
_made = {}


def case(name):
    """The case, made once (treat it as read-only)."""
    if name not in _made:
        _made[name] = CASES[name]()
    return _made[name]


def tables_only(cands):
    """The population with every 1-D row as a 1 x 4 table: what pick_spots_by_intensities accepts."""
    return [[np.array(e).reshape(-1, 4) if len(e) else [] for e in regions] for regions in cands]


def cum_table(n, seed=0):
    """``n`` sorted values and targets for them: below the first, above the last, stored values, values between and NaN."""
    rs = np.random.RandomState(seed + n)
    v = np.sort(rs.uniform(0, 1000, n))
    pick = v[rs.randint(0, n, min(n, 200))]
    t = np.concatenate([[v[0] - 1, v[0], v[-1], v[-1] + 1, np.nan, -np.inf, np.inf], pick, pick + 1e-9,
                        rs.uniform(-10, 1010, 200)])
    return v, t


def golden_meta(gold, name):
    """The JSON record of a case in tests/golden/pick.npz: ``diff``, ``text``, ``keys`` / ``lengths`` of the reference arrays
    per kind, and ``digests`` of every array of the case (pick_ref.digest)."""
    return json.loads(str(gold[name + "_meta"]))
