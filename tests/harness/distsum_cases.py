"""Deterministic cases of the population distance summaries (csrc/distsum.hip), shared by scripts/make_distsum_golden.py and
the tests.  A flat case is N pairs of coordinate tables: ``a`` (N, Ra, 3) and ``b`` (N, Rb, 3), or ``b = None`` for the cis
map of ``a`` (squareform(pdist) per copy, literal zero diagonal); ``th`` is its contact threshold.  The shapes are the
smallest at which the kernels can go wrong: they own output tiles of 2 x 2, 4 x 4, 8 x 8 (median) or 16 x 16 (mean, counts)
entries and stage 256, 64, 32 and 32 stack entries at a time, so N crosses 32, 64 and 128, fills every chunk exactly at 256,
ends one past every chunk at 257 and at 641 lies past NumPy's switch of nanmedian paths at 600 (two whole chunks of 256
and a part, one past a chunk of 32 and of 64); 19 x 21 straddles every tile in both directions."""
import numpy as np

TH_DEFAULT = 500.0


def _random(seed, N, Ra, Rb, nan=0.3, cis=False, scale=400.0):
    rs = np.random.RandomState(seed)
    a = rs.normal(0.0, scale, (N, Ra, 3))
    a[rs.rand(N, Ra) < nan] = np.nan
    if cis:
        return a, None
    b = rs.normal(0.0, scale, (N, Rb, 3)) + np.array([150.0, 0.0, -80.0])
    b[rs.rand(N, Rb) < nan] = np.nan
    return a, b


def _count_edges():
    """Entries with 0, 1, 2, 3 (odd) and 6 (even) finite values: row r of ``a`` is finite in the first (0, 1, 2, 3, 6)[r]
    copies only."""
    a, b = _random(31, 6, 5, 7, nan=0.0)
    for r, keep in enumerate((0, 1, 2, 3, 6)):
        a[keep:, r] = np.nan
    return a, b


def _ties():
    """Coordinates on a coarse integer grid: most entries have equal values around the middle (lo == hi)."""
    rs = np.random.RandomState(32)
    a = rs.randint(0, 3, (64, 5, 3)).astype(np.float64)
    b = rs.randint(0, 3, (64, 7, 3)).astype(np.float64)
    a[rs.rand(64, 5) < 0.1] = np.nan
    return a, b


def _shared_roots():
    """dz = 1000 for every pair behind a large common offset, dy = 0, dx = 1e-5 * (sqrt(j) + sqrt(k)) with small integers j
    of (n, row) and k of (n, column): the q lie about one ulp of 1e6 apart, so distinct q share a root (the fixture script
    counts such pairs in every entry)."""
    N, Ra, Rb = 64, 5, 7
    j = (np.arange(N)[:, None] * 37 + np.arange(Ra)[None, :] * 11) % 97
    k = (np.arange(N)[:, None] * 29 + np.arange(Rb)[None, :] * 5) % 89
    a, b = np.zeros((N, Ra, 3)), np.zeros((N, Rb, 3))
    a[:, :, 0] = 1.0e6 + 1000.0
    b[:, :, 0] = 1.0e6
    a[:, :, 1] = 1.0e-5 * np.sqrt(j.astype(np.float64))
    b[:, :, 1] = -1.0e-5 * np.sqrt(k.astype(np.float64))
    return a, b


def _infinite():
    """Plain inf (an infinite distance, not finite, a value of the median) and inf - inf (NaN)."""
    a, b = _random(33, 5, 5, 7, nan=0.0)
    a[0, 0, 0] = np.inf          # against finite b: inf; against b[0, 0]: inf - inf
    b[0, 0, 0] = np.inf
    a[1:4, 1, 2] = np.inf        # three of five values of row 1 infinite: the median is inf
    b[2, 3, 1] = -np.inf
    a[4, 2] = np.nan
    return a, b


def coords_for_q(target, dz):
    """dx with fl(fl(dz * dz) + fl(dx * dx)) == target, found by stepping dx in ulps (dz * dz < target)."""
    zz = dz * dz
    dx = np.sqrt(target - zz)
    for step in range(-2000, 2001):
        x = dx
        for _ in range(abs(step)):
            x = np.nextafter(x, np.inf if step > 0 else -np.inf)
        if zz + x * x == target:
            return x
    raise AssertionError("no dx for q = %r" % target)


def qstar(th):
    """The largest double whose root is <= th (csrc/ia3_distsum.h says the same in C)."""
    th = np.float64(th)
    if not th >= 0:
        return np.float64(-1.0)
    if th == np.inf:
        return np.float64(np.inf)
    with np.errstate(over="ignore"):
        c = th * th
    while np.sqrt(c) > th:
        c = np.nextafter(c, -np.inf)
    while True:
        up = np.nextafter(c, np.inf)
        if up == np.inf or not np.sqrt(up) <= th:
            return c
        c = up


def _contact(th, dz):
    """Row r of ``a`` against column 0 of ``b`` (the origin) has q = q* - 1 ulp, q*, q* + 1 ulp for r = 0, 1, 2 in every
    copy; row 3 is at a distance of exactly ``th`` where that is possible (th = 5: the 3-4-5 triangle); the other entries
    are random around the threshold."""
    rs = np.random.RandomState(int(th * 10))
    N, Ra, Rb = 5, 5, 7
    a = rs.normal(0.0, th, (N, Ra, 3))
    b = rs.normal(0.0, th, (N, Rb, 3))
    b[:, 0] = 0.0
    qs = qstar(th)
    for r, t in enumerate((np.nextafter(qs, -np.inf), qs, np.nextafter(qs, np.inf))):
        a[:, r] = [dz, coords_for_q(t, dz), 0.0]
    if th == 5.0:
        a[:, 3] = [3.0, 4.0, 0.0]
    a[4, 4] = np.nan
    return a, b


def _build(name):
    if name.startswith("r_"):       # r_<N>_<Ra>x<Rb> or r_<N>_cis<R>
        _, n, shape = name.split("_")
        N = int(n)
        if shape.startswith("cis"):
            R = int(shape[3:])
            return _random(100 + N + R, N, R, R, cis=True)
        Ra, Rb = [int(v) for v in shape.split("x")]
        return _random(100 + N + 7 * Ra + Rb, N, Ra, Rb)
    return {"count_edges": _count_edges, "ties": _ties, "shared_roots": _shared_roots, "infinite": _infinite,
            "contact_06": lambda: _contact(0.6, 0.6 - 2.0e-9), "contact_5": lambda: _contact(5.0, 5.0 - 2.0e-8)}[name]()


THRESHOLDS = {"contact_06": 0.6, "contact_5": 5.0, "ties": 2.0, "shared_roots": 1000.0, "infinite": np.inf}

CASES = ("r_1_1x1", "r_9_1x1", "r_129_1x1", "r_641_1x1", "r_1_5x7", "r_2_5x7", "r_63_5x7", "r_64_19x21", "r_65_5x7",
         "r_129_19x21", "r_256_5x7", "r_257_5x7", "r_641_19x21", "r_2_cis5", "r_65_cis19", "count_edges", "ties", "shared_roots", "infinite",
         "contact_06", "contact_5")

_made = {}


def case(name):
    """(a, b or None, th): read-only arrays, made once."""
    if name not in _made:
        a, b = _build(name)
        a.setflags(write=False)
        if b is not None:
            b.setflags(write=False)
        _made[name] = (a, b, THRESHOLDS.get(name, TH_DEFAULT))
    return _made[name]


def as_cells(a, b):
    """The flat case as a chr_2_zxys_list of the reference: chromosome '1' (and '2') with one copy per cell."""
    if b is None:
        return [{'1': [a[n]]} for n in range(len(a))], ('1', '1')
    return [{'1': [a[n]], '2': [b[n]]} for n in range(len(a))], ('1', '2')


# ---- the codebook structure ----------------------------------------------------------------------------------------------------

STRUCT_REGIONS = {'1': 5, '2': 7, 'X': 4}
STRUCT_TH = 500.0


def struct_codebook():
    """Columns of the codebook as arrays (``codebook['chr']`` is all the summaries read); 'X' is a chromosome no cell has."""
    chrs = np.array(['2'] * 3 + ['1'] * 5 + ['X'] * 4 + ['2'] * 4)
    order = np.zeros(len(chrs), dtype=np.int64)
    for c in np.unique(chrs):
        order[chrs == c] = np.arange((chrs == c).sum())
    return {'chr': chrs, 'id': np.arange(len(chrs)) + 10, 'chr_order': order}


def struct_cells():
    """12 cells: chromosome '1' with one, two or three homologs (six permutations), absent in cell 3 and None in cell 4;
    chromosome '2' with two homologs, absent in cells 5 and 6, None in cell 7; NaN rows at 30 %."""
    rs = np.random.RandomState(77)

    def table(R):
        t = rs.normal(0.0, 400.0, (R, 3))
        t[rs.rand(R) < 0.3] = np.nan
        return t

    cells = []
    for i in range(12):
        d = {}
        if i == 4:
            d['1'] = None
        elif i != 3:
            d['1'] = [table(5) for _ in range((1, 2, 3)[i % 3])]
        if i == 7:
            d['2'] = None
        elif i not in (5, 6):
            d['2'] = [table(7) for _ in range(2)]
        cells.append(d)
    return cells


STRUCT_KEYS = ["cis_1", "trans_1", ("1", "2"), ("1", "X"), "cis_2", "trans_2", ("2", "X"), "cis_X", "trans_X"]


def key_name(key):
    return key if isinstance(key, str) else "%s-%s" % key


def plot_codebooks():
    """(total, selected) codebooks of the plotting-order helpers as pandas DataFrames: the selection drops some regions and
    keeps its own row numbering."""
    import pandas as pd
    chrs = ['2', '1', '1', 'X', '2', '10', '1', 'X', '2', '10']
    total = pd.DataFrame({'id': [5, 3, 8, 1, 9, 4, 7, 2, 6, 0], 'chr': chrs})
    total['chr_order'] = 0
    for c in set(chrs):
        rows = total.index[total['chr'] == c]
        total.loc[rows, 'chr_order'] = np.arange(len(rows))
    sel = total[total['id'].isin([3, 8, 9, 4, 2, 6, 5])].reset_index(drop=True)
    return total, sel
