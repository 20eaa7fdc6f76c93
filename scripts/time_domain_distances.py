"""Times the domain distances (csrc/domain.hip) on an experiment-sized workload.

    python scripts/time_domain_distances.py [--copies 4000] [--runs 3] [--out profiles/domain_distances.json]
    python scripts/time_domain_distances.py --cpu-reference [--fraction 100]

The workload: `--copies` chromosome copies of 1000 loci (a Gaussian walk, 10 % of the loci NaN), the sliding-window
distances for the window sizes 5..9 with the 'median' metric (what Domain_Calling_Sliding_Window asks for at
window_size 5), domain_pdists for 50 domains per copy (random starts, 1225 pairs each) and the contact frequencies of the
same partition.

Without --cpu-reference (needs the GPU): the upload, then per call the median over the runs of the wall time of the flat
form (host glue, library call, download) and of the HIP-event time of its kernel.  The first copy is held against the NumPy
statement of tests/harness/domain_cases.py bit for bit.

With --cpu-reference (no GPU): that NumPy statement (the reference's procedure: Python loops around np.median) on one core
for `--copies` / `--fraction` copies.  Both parts write into the same JSON file.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

R, WDS, N_DOMAINS = 1000, [5, 6, 7, 8, 9], 50


def make_copies(n, seed=0):
    rs = np.random.RandomState(seed)
    z = np.cumsum(rs.normal(0, 120, (n, R, 3)), axis=1)
    z[rs.rand(n, R) < 0.1] = np.nan
    return z


def make_starts(n, seed=1):
    rs = np.random.RandomState(seed)
    return [np.concatenate([[0], np.sort(rs.choice(np.arange(1, R), N_DOMAINS - 1, replace=False))]) for _ in range(n)]


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
    ap.add_argument("--copies", type=int, default=4000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--fraction", type=int, default=100)
    ap.add_argument("--cpu-reference", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "domain_distances.json"))
    a = ap.parse_args()
    from harness import domain_cases as K
    if a.cpu_reference:
        n = max(1, a.copies // a.fraction)
        z, starts = make_copies(n), make_starts(n)
        t0 = time.perf_counter()
        maps = [K.distance_map(c) for c in z]
        t_maps = time.perf_counter() - t0
        t0 = time.perf_counter()
        for m in maps:
            for wd in WDS:
                K.np_window(m, wd, 'median')
        t_win = time.perf_counter() - t0
        t0 = time.perf_counter()
        for c, s in zip(z, starts):
            K.np_domain_pdists(c, list(s), 'median')
        t_pd = time.perf_counter() - t0
        res = dict(copies=n, distance_maps_s=t_maps, windows_s=t_win, pdists_s=t_pd)
        print(json.dumps(res))
        merge(a.out, "numpy_one_core", res)
        return
    from imageanalysis3_amd import _lib as L
    from imageanalysis3_amd.domain_tools import distance as D
    L.check(L.lib().ia3_init(0))
    z, starts = make_copies(a.copies), make_starts(a.copies)
    t0 = time.perf_counter()
    pop = L.DomainPopulation.upload(z)
    t_upload = time.perf_counter() - t0
    calls = [("windows", "domain_slide", lambda: D.population_sliding_window_dists(pop, WDS, 'median')),
             ("pdists", "domain_dists", lambda: D.population_domain_pdists(pop, starts, 'median')),
             ("contacts", "domain_contacts", lambda: D.population_domain_contact_freq(pop, starts, 400))]
    res = dict(copies=a.copies, loci=R, window_sizes=WDS, domains=N_DOMAINS, upload_s=t_upload,
               window_problems=a.copies * len(WDS) * R, pairs=a.copies * N_DOMAINS * (N_DOMAINS - 1) // 2)
    first = {}
    for name, kernel, call in calls:
        call()                                              # warm
        walls, kernels = [], []
        for _ in range(a.runs):
            L.profile_enable(True)
            L.profile_collect()
            t0 = time.perf_counter()
            out = call()
            walls.append(time.perf_counter() - t0)
            kernels.append(L.profile_collect()[kernel][1] * 1e-3)
            L.profile_enable(False)
        res[name + "_wall_s"], res[name + "_kernel_s"] = float(np.median(walls)), float(np.median(kernels))
        first[name] = out[0]
    pop.free()
    m0 = K.distance_map(z[0])
    assert K.same(first["windows"], np.array([K.np_window(m0, wd, 'median') for wd in WDS]))
    assert K.same(first["pdists"], K.np_domain_pdists(z[0], list(starts[0]), 'median').astype(np.float64))
    assert K.same(first["contacts"], K.np_contact_freq(z[0], list(starts[0]), 400))
    print(json.dumps(res))
    merge(a.out, "mi355x", res)


if __name__ == "__main__":
    main()
