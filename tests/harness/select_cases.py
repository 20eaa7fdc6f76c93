"""Inputs of the chromosome-selection tests (tests/test_select_chromosomes_cpu.py, tests/test_gpu_select_chromosomes.py,
scripts/make_select_golden.py): seeded, nothing stored.

A case is ``(cands, spots_list, intensity_th, loss_th)``: candidate centres in pixels ((C, 3), or a list of C arrays),
one spot table per round with the columns [intensity, z, x, y, row id] (the row id lets an assignment be stored as index
arrays), and the two thresholds.  Coordinates sit on the integer pixel lattice, so that scaled by (200, 108, 108) every
squared distance below 2^53 is exact and exact ties are common.
"""
import numpy as np

THREADS, TILE = 256, 256          # workgroup size and candidate tile of csrc/select.hip (_lib.SELECT_THREADS / SELECT_TILE)
VOLUME = (30, 256, 256)
DISTANCE_ZXY = (200, 108, 108)


def _table(rows, dtype=np.float64):
    """Spot table of ``rows`` = [(intensity, z, x, y), ...] with the row id as fifth column."""
    t = np.zeros((len(rows), 5), dtype=dtype)
    if len(rows):
        t[:, :4] = np.asarray(rows, dtype=np.float64)
        t[:, 4] = np.arange(len(rows))
    return t


def lattice(seed, n_cand, n_rounds, selected_per_round, spurious=0, duplicates=0, intensity_th=0.5, loss_th=0.4,
            dtype=np.float64, dropped=3):
    """``n_cand`` candidates on the lattice of VOLUME (the last ``duplicates`` repeat earlier rows, the ``spurious`` before
    them show a spot in one round of five), and per round exactly ``selected_per_round`` rows at or above the threshold,
    most of them within 2 pixels of a candidate that is present in that round, the rest anywhere; ``dropped`` more rows
    lie below the threshold or have a NaN intensity."""
    rs = np.random.RandomState(seed)
    cands = np.stack([rs.randint(0, s, n_cand) for s in VOLUME], axis=1).astype(np.float64)
    for k in range(duplicates):
        cands[n_cand - 1 - k] = cands[rs.randint(0, max(1, n_cand - duplicates))]
    p_present = np.full(n_cand, 0.9)
    p_present[n_cand - duplicates - spurious:n_cand - duplicates] = 0.2
    spots_list = []
    for r in range(n_rounds):
        rows = []
        present = np.flatnonzero(rs.rand(n_cand) < p_present)
        for k in range(selected_per_round):
            if len(present) and k < 0.85 * selected_per_round:
                c = cands[present[k % len(present)]]
                zxy = c + rs.randint(-2, 3, 3)
            else:
                zxy = [rs.randint(0, s) for s in VOLUME]
            rows.append((0.5 + rs.randint(0, 8) * 0.25, zxy[0], zxy[1], zxy[2]))    # 0.5 itself is selected (>=)
        for k in range(dropped):
            zxy = [rs.randint(0, s) for s in VOLUME]
            rows.append(((0.25, np.nan, 0.49)[k % 3], zxy[0], zxy[1], zxy[2]))
        order = rs.permutation(len(rows))
        spots_list.append(_table([rows[i] for i in order], dtype))
    return cands, spots_list, intensity_th, loss_th


def _no_spot():
    """Three candidates and three rounds without a selected spot (an empty table, every row below the threshold, NaN
    intensities): every candidate is lost everywhere, all are removed in index order and the reference's max() fails."""
    cands = np.array([[3, 10, 10], [5, 40, 40], [7, 80, 90]], dtype=np.float64)
    spots_list = [np.zeros((0, 5)), _table([(0.1, 3, 10, 10), (0.49, 5, 40, 40)]), _table([(np.nan, 7, 80, 90)])]
    return cands, spots_list, 0.5, 0.4


def _one_spot():
    """One round, one spot, three candidates: the two that do not own it go, one is left."""
    cands = np.array([[3, 10, 10], [5, 40, 40], [7, 80, 90]], dtype=np.float64)
    return cands, [_table([(1.0, 5, 41, 40)])], 0.5, 0.4


def _chain():
    """Ten rounds on a line y = const.  Z (y = 200) has a spot in every round.  X (y = 10) has spots at y = 9 in rounds
    0-3 (lost 6), Y (y = 20) has spots at y = 16 in rounds 4-6 (lost 7), W (y = 120) has none (lost 10).  W goes first and
    moves nothing; then Y goes, its spots fall to X (6 pixels away, Z is 184), X gains rounds 4-6 (lost 3) and stays."""
    cands = np.array([[5, 50, 10], [5, 50, 20], [5, 50, 200], [5, 50, 120]], dtype=np.float64)
    spots_list = []
    for r in range(10):
        rows = [(1.0, 5, 50, 199 + r % 3)]
        if r < 4:
            rows.append((0.75, 5, 50, 9))
        if 4 <= r < 7:
            rows.append((2.0, 5, 50, 16))
        spots_list.append(_table(rows))
    return cands, spots_list, 0.5, 0.4


def _odd_values():
    """NaN and +-inf coordinates in selected rows: a NaN makes the whole row of distances NaN (first candidate), an
    infinity makes them all inf or NaN."""
    cands, spots_list, a, b = lattice(71, 5, 6, 12)
    bad = [(np.nan, 4, 4), (3, np.inf, 4), (3, 4, -np.inf), (np.inf, np.nan, 2), (-np.inf, np.inf, np.inf)]
    for r, t in enumerate(spots_list):
        sel = np.flatnonzero(t[:, 0] >= a)
        t[sel[r % len(sel)], 1:4] = bad[r % len(bad)]
        t[sel[(r + 3) % len(sel)], 1:4] = bad[(r + 2) % len(bad)]
    return cands, spots_list, a, b


def _equal_roots():
    """Two candidates whose squared distances from the spots at the origin differ and whose roots are equal: with
    j = 3 t, k = 4 t the lattice points (0, j + 4, k - 3) and (0, j, k) have j^2 + k^2 + 25 and j^2 + k^2.  The FIRST
    candidate has the larger sum: np.argmin keeps it, a comparison of the sums would hand every spot to the second.  A third
    candidate far away never owns a spot."""
    d = float(DISTANCE_ZXY[1])
    for t in range(100000000, 100004000):
        a = np.array([(3 * t + 4) * d, (4 * t - 3) * d])
        b = np.array([(3 * t) * d, (4 * t) * d])
        sa, sb = (0.0 + a[0] * a[0]) + a[1] * a[1], (0.0 + b[0] * b[0]) + b[1] * b[1]
        if sa > sb and np.sqrt(sa) == np.sqrt(sb):
            break
    else:
        raise AssertionError("no pair of unequal sums with equal roots")
    cands = np.array([[0, 3 * t + 4, 4 * t - 3], [0, 3 * t, 4 * t], [0, -8 * t, 0]], dtype=np.float64)
    spots_list = [_table([(1.0, 0, 0, 0), (0.5, 0, 0, 0)]) for r in range(3)]
    return cands, spots_list, 0.5, 0.4


def _gaps():
    """Rounds without a selected spot between rounds that have some: the first round is an empty table, round 3 lies below
    the threshold, round 4 (next to it: a start repeated twice) and the last round have NaN intensities.  Those 4 of 14
    rounds are lost for every candidate; the spurious candidates go, the others stay."""
    cands, spots_list, a, b = lattice(17, 8, 14, 24, spurious=3)
    spots_list[0] = np.zeros((0, 5))
    spots_list[3][:, 0] = 0.25
    spots_list[4][:, 0] = np.nan
    spots_list[13][:, 0] = np.nan
    return cands, spots_list, a, b


def _as_list(case):
    cands, spots_list, a, b = case
    return [np.array(c) for c in cands], spots_list, a, b


# name -> builder.  Candidate counts 1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 TILE + 37; selected spots 0, 1,
# THREADS - 1, THREADS, THREADS + 1 (one round each) and 30 x 680; R = 1 and R = 40.
CASES = {
    "c1": lambda: lattice(1, 1, 3, 6),
    "c2": lambda: lattice(2, 2, 4, 9, spurious=1),
    "c63": lambda: lattice(3, 63, 5, 70, spurious=6, duplicates=2),
    "c64": lambda: lattice(4, 64, 5, 70, spurious=6),
    "c65": lambda: lattice(5, 65, 5, 70, spurious=6, duplicates=1),
    "tile_less": lambda: lattice(6, TILE - 1, 6, 300, spurious=8),
    "tile": lambda: lattice(7, TILE, 6, 300, spurious=8),
    "tile_more": lambda: lattice(8, TILE + 1, 6, 300, spurious=8, duplicates=2),
    "big": lambda: lattice(9, 2 * TILE + 37, 30, 680, spurious=10, duplicates=2),
    "r40": lambda: lattice(16, 12, 40, 20, spurious=3),
    "s0": _no_spot,
    "s1": _one_spot,
    "wg_less": lambda: lattice(10, 7, 1, THREADS - 1, spurious=2),
    "wg": lambda: lattice(11, 7, 1, THREADS, spurious=2),
    "wg_more": lambda: lattice(12, 7, 1, THREADS + 1, spurious=2),
    "chain": _chain,
    "th_zero": lambda: lattice(13, 6, 8, 10, spurious=3, loss_th=0.0),
    "odd_values": _odd_values,
    "float32": lambda: lattice(14, 20, 7, 40, spurious=4, dtype=np.float32),
    "cand_list": lambda: _as_list(lattice(15, 9, 5, 30, spurious=2, duplicates=1)),
    "equal_roots": _equal_roots,
    "gaps": _gaps,
}
RAISES = ("s0",)                  # the cases in which the last candidate is removed
LITERAL_SLOW = ("big",)           # the literal loop of these runs for seconds: the reference's own run (the golden) stands for it


def case(name):
    return CASES[name]()
