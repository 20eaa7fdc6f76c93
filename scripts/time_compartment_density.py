"""Times the compartment densities (csrc/density.hip) on an experiment-sized workload.

    python scripts/time_compartment_density.py [--cells 2000] [--runs 3] [--out profiles/compartment_density.json]
    python scripts/time_compartment_density.py --cpu-reference [--fraction 100]

The workload: `--cells` nuclei of 20 chromosomes x 2 homologs x 60 regions (2 400 loci each, 10 % of them NaN), 25 regions
of every chromosome labelled A and 25 B, trans alone, one sigma of 500 nm.

Without --cpu-reference (needs the GPU): the packing of the cells on the host and the upload (the creation), one scoring
call warm (median over the runs: wall time of the library call and HIP-event time of its kernel), and ten calls with
shuffled labels on the resident population.  Reported: weighted pairs per second (a pair is one evaluated exp; their number
is the sum of the returned counts, the labels being disjoint) and the float64 vector instructions they take as a fraction
of the peak of 256 compute units x 64 lanes x 2.4 GHz.  The instruction count per weighted pair, 64, is read off the gfx950
disassembly of density_k: 43 for the argument (three IEEE divisions of 11 each), 18 for exp, 3 for the weighted add.  The
first cell is held against the NumPy restatement below to 1e-12.

With --cpu-reference (no GPU): the reference's procedure restated with NumPy (per query: gather the contributing rows,
drop the rows that are not finite, exp, sum) on one core for `--cells` / `--fraction` cells.  Both parts write into the
same JSON file.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CHRS = [str(i + 1) for i in range(20)]
H, R, SIGMA = 2, 60, 500.0
INSTR_PER_PAIR = 64
PEAK_LANE_OPS = 256 * 64 * 2.4e9


def make_cells(n, seed=0):
    rs = np.random.RandomState(seed)
    cells = []
    for _ in range(n):
        cell = {}
        for c in CHRS:
            z = rs.uniform(-3000, 3000, (H, 1, 3)) + np.cumsum(rs.normal(0, 150, (H, R, 3)), axis=1)
            z[rs.rand(H, R) < 0.1] = np.nan
            cell[c] = z
        cells.append(cell)
    return cells


def make_labels(seed):
    rs = np.random.RandomState(seed)
    out = {}
    for c in CHRS:
        p = rs.permutation(R)
        out[c] = {'A': np.sort(p[:25]), 'B': np.sort(p[25:50])}
    return out


def numpy_cell(cell, labels, sigma):
    """density.py:11-87 for trans alone, unnormalised, restated: chr -> {'A': (H, R), 'B': (H, R)}."""
    s2 = np.array(sigma, dtype=float)**2
    out = {}
    for c, zxys in cell.items():
        res = {k: np.zeros(zxys.shape[:2]) for k in 'AB'}
        for h, copy in enumerate(zxys):
            for r, q in enumerate(copy):
                if np.isnan(q).any():
                    res['A'][h, r] = res['B'][h, r] = np.nan
                    continue
                for k in 'AB':        # the rows are gathered anew for every query, as the reference does
                    rows = np.concatenate([other[labels[c2][k]] for c2, zs in cell.items() for h2, other in enumerate(zs)
                                           if c2 != c or h2 != h])
                    rows = rows[np.isfinite(rows).all(1)]
                    res[k][h, r] = np.exp(-0.5 * np.sum((rows - q)**2 / s2, axis=-1)).sum()
        out[c] = res
    return out


def merge(path, key, value):
    res = {}
    if os.path.isfile(path):
        with open(path) as f:
            res = json.load(f)
    res[key] = value
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=2000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--fraction", type=int, default=100)
    ap.add_argument("--cpu-reference", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compartment_density.json"))
    a = ap.parse_args()
    labels = make_labels(1)
    if a.cpu_reference:
        n = max(1, a.cells // a.fraction)
        cells = make_cells(a.cells if a.cells < 64 else 64)[:n]
        t0 = time.perf_counter()
        for cell in cells:
            numpy_cell(cell, labels, SIGMA)
        dt = time.perf_counter() - t0
        res = dict(cells=n, seconds=dt, seconds_per_cell=dt / n)
        print(json.dumps(res))
        merge(a.out, "numpy_one_core", res)
        return
    from imageanalysis3_amd import _lib as L
    from imageanalysis3_amd.compartment_tools import density as D
    L.check(L.lib().ia3_init(0))
    cells = make_cells(a.cells)
    t0 = time.perf_counter()
    layout = L.DensityLayout(cells, labels)
    t_pack = time.perf_counter() - t0
    t0 = time.perf_counter()
    pop = L.DensityPopulation.upload(layout, None)
    t_upload = time.perf_counter() - t0
    D.population_compartment_densities(pop, labels, SIGMA)          # warm
    walls, kernels = [], []
    for _ in range(a.runs):
        L.profile_enable(True)
        L.profile_collect()
        t0 = time.perf_counter()
        sums, counts = D.population_compartment_densities(pop, labels, SIGMA, return_counts=True)
        walls.append(time.perf_counter() - t0)
        kernels.append(L.profile_collect()["density"][1] * 1e-3)
        L.profile_enable(False)
    wall, kernel = float(np.median(walls)), float(np.median(kernels))
    pairs = int(counts.astype(np.int64).sum())
    t0 = time.perf_counter()
    for k in range(10):
        D.population_compartment_densities(pop, make_labels(100 + k), SIGMA)
    t_shuffled = time.perf_counter() - t0
    want = numpy_cell(cells[0], labels, SIGMA)
    first = np.stack([np.concatenate([want[c][k].ravel() for c in want]) for k in 'AB'])
    mine = sums[:, :first.shape[1]]
    ok = ~np.isnan(first)
    assert np.array_equal(np.isnan(mine), np.isnan(first)) and (np.abs(mine[ok] - first[ok]) <= 1e-12 * first[ok] + 2e-305).all()
    pop.free()
    res = dict(cells=a.cells, loci=int(layout.n_points), weighted_pairs=pairs, pack_s=t_pack, upload_s=t_upload,
               score_wall_s=wall, score_kernel_s=kernel, ten_shuffled_s=t_shuffled, pairs_per_s=pairs / kernel,
               fp64_vector_fraction=pairs / kernel * INSTR_PER_PAIR / PEAK_LANE_OPS, instructions_per_pair=INSTR_PER_PAIR)
    print(json.dumps(res))
    merge(a.out, "mi355x", res)


if __name__ == "__main__":
    main()
