"""Deterministic cases of the compartment densities (csrc/density.hip), shared by scripts/make_density_golden.py and the
tests.  A cell is a dict ``chr -> (H, R, 3)``; ``AB`` is the one ``chr_2_AB_dict`` of all cells.  The genome has chromosomes
of 1, 2, 7, 16 and 60 regions so that a number of homologs per chromosome gives a cell any total of loci.  The kernel gives
a workgroup 128 queries, stages 256 contributors and sums them in parts of 64; the totals cross the edges of any tile of 32
to 256 (31, 32, 33 ... 255, 256, 257), 600 has five query tiles and three contributor tiles, 1 100 nine and five."""
import itertools

import numpy as np

REGIONS = {'a': 1, 'b': 2, 'c': 7, 'd': 16, 'e': 60}      # the chromosomes and their regions
ORDER = ('e', 'd', 'c', 'b', 'a')                         # a total is made greedily, the longest chromosome first
SIGMAS = {"scalar": 300.0, "aniso": [450.0, 300.0, 250.0]}
SIGMA_X = 300.0                                           # the x sigma of both


def _labels():
    rs = np.random.RandomState(70)
    e = rs.permutation(60)
    d = rs.permutation(16)
    return {
        'a': {'A': np.array([0]), 'B': np.array([], dtype=np.int64)},
        'b': {'A': [0], 'B': [1]},                                             # plain lists
        'c': {'A': np.array([0, 2, 4, 4]), 'B': np.array([1, 3])},             # 4 twice; 5 and 6 in neither class
        'd': {'A': np.sort(d[:7]), 'B': np.sort(np.concatenate([d[6:12], d[8:9]]))},     # d[6] in both, d[8] twice in B
        'e': {'A': np.sort(np.concatenate([e[:25], e[3:5]])), 'B': e[25:50]},  # two duplicates, B unsorted, ten in neither
    }


AB = _labels()

SMALL_TOTALS = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129)
LARGE_TOTALS = (255, 256, 257, 600, 1100)
TOTALS = SMALL_TOTALS + LARGE_TOTALS


def homologs(total):
    """chr -> H of a cell of ``total`` loci."""
    out, left = {}, total
    for c in ORDER:
        h, left = divmod(left, REGIONS[c])
        if h:
            out[c] = h
    return out


def _cell(seed, hom, nan=0.0, scale=600.0):
    rs = np.random.RandomState(seed)
    cell = {}
    for c, h in hom.items():
        centre = rs.normal(0.0, scale, (h, 1, 3))
        z = centre + rs.normal(0.0, 0.5 * scale, (h, REGIONS[c], 3))
        z[rs.rand(h, REGIONS[c]) < nan] = np.nan
        cell[c] = z
    return cell


def far_cell():
    """Two homologs of 'd' as two tight clusters 37 to 39.5 sigma apart along x: with trans alone every term lies between
    the last normal numbers and below the smallest subnormal (exp(-708.4) at 37.6 sigma, exp(-745.1) at 38.6)."""
    rs = np.random.RandomState(71)
    z = rs.normal(0.0, 0.01 * SIGMA_X, (2, 16, 3))
    z[1, :, 1] += SIGMA_X * np.linspace(37.0, 39.5, 16)
    return {'d': z}


def cells():
    """The population of the GPU test: one cell per total, then a cell whose every locus is NaN and the far cell.
    The cell of 129 loci holds NaN loci, an inf coordinate, the duplicated indices, the regions in neither class and
    single-homolog chromosomes; the cells of 1 and 2 loci hold one copy (trans alone gives NaN)."""
    out = []
    for i, t in enumerate(TOTALS):
        out.append(_cell(100 + i, homologs(t), nan=0.12 if t in (129, 600) else 0.0))
    out[TOTALS.index(129)]['e'][1, 7, 2] = np.inf
    out[TOTALS.index(129)]['c'][0, 4, 0] = -np.inf         # a contributor listed twice
    out[TOTALS.index(600)]['e'][3, 20, 1] = np.inf
    dark = _cell(200, homologs(33))
    for c in dark:
        dark[c][:] = np.nan
    out.append(dark)
    out.append(far_cell())
    return out


N_SMALL = len(SMALL_TOTALS)                # cells()[i] for i < N_SMALL and the last two have the full option matrix


def small_indices():
    return list(range(N_SMALL)) + [len(TOTALS), len(TOTALS) + 1]


def large_indices():
    return list(range(N_SMALL, len(TOTALS)))


def option_name(use_cis, use_trans, exclude_self, normalize, sigma):
    return "c%dt%dx%dn%d_%s" % (use_cis, use_trans, exclude_self, normalize, sigma)


def full_options():
    """(use_cis, use_trans, exclude_self, normalize_by_reg_num, sigma name): the 24 option sets."""
    return [(c, t, x, n, s) for (c, t), x, n, s in itertools.product(((0, 1), (1, 0), (1, 1)), (0, 1), (0, 1), ("scalar", "aniso"))]


LARGE_OPTIONS = [(0, 1, 1, 0, "scalar"), (1, 0, 1, 1, "aniso"), (1, 1, 0, 0, "aniso"), (1, 1, 1, 1, "scalar")]


def flat(dicts):
    """(2, points) of a list of per-cell result dicts, in the population's point order."""
    return np.stack([np.concatenate([d[c][k].ravel() for d in dicts for c in d]) for k in ('A', 'B')])


def gaussian_case():
    """centers (70, 3) with a NaN row, an inf row and a far row; ref_center; (sigma, intensity, background) triples."""
    rs = np.random.RandomState(72)
    centers = rs.normal(0.0, 400.0, (70, 3))
    centers[5] = np.nan
    centers[9, 1] = np.inf
    centers[11] = [0.0, 38.0 * SIGMA_X, 0.0]
    ref = rs.normal(0.0, 100.0, 3)
    return centers, ref, [(300.0, 1, 0), ([450.0, 300.0, 250.0], 2.5, 10), (np.float32(200.0), 1, -1)]


def arg_case():
    """Rows of (contributor z x y, query z x y, sigma z x y) for the bit-exact check of the argument of exp; the squared
    sigmas are NumPy's ``sigma**2``."""
    rs = np.random.RandomState(73)
    n = 4096
    v = np.empty((n, 9))
    v[:, :6] = rs.normal(0.0, 800.0, (n, 6))
    v[:, 6:] = rs.uniform(50.0, 600.0, (n, 3))
    v[:64, 3:6] = v[:64, :3] + rs.normal(0.0, 1e-3, (64, 3))     # near pairs
    v[64:128, 1] += 38.0 * v[64:128, 7]                          # far pairs
    v[128, 3] = np.inf
    v[129, 0] = np.nan
    v[130, 6] = 0.0                                              # sigma 0: inf, or NaN for a zero difference
    v[131, 6], v[131, 0] = 0.0, v[131, 3]
    return v


def weight_table():
    """The per-pair weight for every (flags, same copy, self, multiplicity in 0, 1, 3), in the order the native program
    prints it: flags bit 0 use_cis, bit 1 use_trans, bit 2 exclude_self."""
    rows = []
    for flags in range(8):
        cis, trans, excl = flags & 1, flags & 2, flags & 4
        for same in (0, 1):
            for self_ in (0, 1):
                for mult in (0, 1, 3):
                    if not same:
                        w = mult if trans else 0
                    else:
                        w = 1 if (cis and mult > 0 and not (self_ and excl)) else 0
                    rows.append((flags, same, self_, mult, w))
    return rows
