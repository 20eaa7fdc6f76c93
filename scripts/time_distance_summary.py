"""Times the population distance summaries (csrc/distsum.hip) on two experiment-sized workloads.

    python scripts/time_distance_summary.py [--copies 2000] [--regions 1000] [--runs 3] [--out profiles/distance_summary.json]
    python scripts/time_distance_summary.py --cpu-reference [--fraction 100]

The workloads:
  cis     one cis key: `--copies` random-walk chromosomes of `--regions` regions, 10 % of the rows NaN; the nanmedian
          map, and the nanmean and contact maps (threshold 500 nm) for comparison
  genome  a genome-wide set: 20 chromosomes x 60 regions, 2000 cells x 2 homologs, all 230 keys of
          Chr2ZxysList_2_summaryDict (cis and trans of every chromosome: 4000 matrices each; every pair: 8000)

Without --cpu-reference (needs the GPU): the upload once, then every call warm, median over the runs: the wall time of the
library call (pair validation, the 2 N ints up, the kernels, the maps down, one synchronise) and the HIP-event time of its
kernels (ia3_profile_*), so the share of the kernels in the call is measured, not assumed.  The cis median is held against
the NumPy statement (tests/harness/distsum_ref.py) on its first 40 x 40 entries, bit for bit.  For the genome set the wall
time of the whole function and of its parts: the host's tables and pair lists, the upload, the device calls.

With --cpu-reference (no GPU): SciPy's squareform(pdist) per copy and np.nanmedian of the stack, the reference's own
expressions, on one core for the first regions / sqrt(`--fraction`) regions of the cis workload, that is 1 / `--fraction`
of its distances.  Both parts write into the same JSON file.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def walks(n, R, seed):
    rs = np.random.RandomState(seed)
    t = rs.uniform(2000, 40000, (n, 1, 3)) + np.cumsum(rs.normal(0, 300, (n, R, 3)), axis=1)
    t[rs.rand(n, R) < 0.1] = np.nan
    return t


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


def timed(L, call, runs, prefix="dist_"):
    """(median wall ms, median kernel ms per ProfScope name) of a warm call."""
    call()
    walls, kernels = [], []
    for _ in range(runs):
        L.profile_enable(True)
        L.profile_collect()
        t0 = time.perf_counter()
        call()
        walls.append((time.perf_counter() - t0) * 1e3)
        prof = L.profile_collect()
        L.profile_enable(False)
        kernels.append({k: v[1] for k, v in prof.items() if k.startswith(prefix)})
    names = sorted(set(k for d in kernels for k in d))
    return float(np.median(walls)), {k: float(np.median([d.get(k, 0.0) for d in kernels])) for k in names}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--copies", type=int, default=2000)
    ap.add_argument("--regions", type=int, default=1000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--fraction", type=int, default=100)
    ap.add_argument("--cells", type=int, default=2000)
    ap.add_argument("--skip-genome", action="store_true")
    ap.add_argument("--cpu-reference", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distance_summary.json"))
    a = ap.parse_args()
    N, R = a.copies, a.regions
    if a.cpu_reference:
        from scipy.spatial.distance import pdist, squareform
        sub = max(1, int(round(R / np.sqrt(a.fraction))))
        t = walks(N, R, 3)[:, :sub]
        t0 = time.perf_counter()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            m = np.nanmedian([squareform(pdist(z)) for z in t], axis=0)
        dt = time.perf_counter() - t0
        out = dict(copies=N, regions=sub, distances=int(N) * sub * sub, share_of_the_cis_workload=sub * sub / float(R * R),
                   seconds=dt, threads=1, checksum=float(np.nansum(m)))
        print(json.dumps(out), flush=True)
        merge(a.out, "scipy_numpy_one_core", out)
        return
    from harness import distsum_ref as S
    from imageanalysis3_amd import _lib as L
    from imageanalysis3_amd.structure_tools import distance as D
    L.check(L.lib().ia3_init(0))
    name = C.create_string_buffer(256)
    L.lib().ia3_device_name(name, 256)
    gpu = name.value.decode()
    # ---- one cis key
    t = walks(N, R, 3)
    t0 = time.perf_counter()
    pop = L.DistancePopulation.upload(list(t))
    upload_ms = (time.perf_counter() - t0) * 1e3
    ids = np.arange(N, dtype=np.int32)
    res = dict(gpu=gpu, copies=N, regions=R, distances=int(N) * R * R, runs=a.runs, upload_ms=upload_ms, upload_bytes=int(t.nbytes))
    for tile in (8, 4, 2):
        L.check(L.lib().ia3_set_tuning(L.IA3_TUNE_DIST_TILE, tile))
        wall, k = timed(L, lambda: pop.summary(ids, ids, function=L.DIST_NANMEDIAN, same=True), a.runs)
        res["median_tile%d" % tile] = dict(call_wall_ms=wall, kernel_ms=k, kernel_share_of_call=sum(k.values()) / wall)
    L.check(L.lib().ia3_set_tuning(L.IA3_TUNE_DIST_TILE, 0))
    med = pop.summary(ids, ids, function=L.DIST_NANMEDIAN, same=True)
    res["median_equal_to_statement_40x40"] = bool(S.same_values(med[:40, :40], S.median(S.q_stack(t[:, :40]))))
    res["median_nan_entries"] = int(np.isnan(med).sum())
    for fname, code in (("mean", L.DIST_NANMEAN), ("contact", L.DIST_CONTACT)):
        wall, k = timed(L, lambda: pop.summary(ids, ids, function=code, contact_th=500.0, same=True), a.runs)
        res[fname] = dict(call_wall_ms=wall, kernel_ms=k, kernel_share_of_call=sum(k.values()) / wall)
    pop.free()
    print(json.dumps(res), flush=True)
    merge(a.out, "cis_key", res)
    if a.skip_genome:
        return
    # ---- a genome-wide set
    chrs, Rg, cells_n = [str(c) for c in range(1, 21)], 60, a.cells
    tabs = walks(cells_n * 2 * len(chrs), Rg, 4).reshape(cells_n, len(chrs), 2, Rg, 3)
    cells = [{c: [tabs[i, j, 0], tabs[i, j, 1]] for j, c in enumerate(chrs)} for i in range(cells_n)]
    book = {'chr': np.repeat(np.array(chrs), Rg)}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        D.Chr2ZxysList_2_summaryDict(cells, book)                                        # warm
        walls = []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            out = D.Chr2ZxysList_2_summaryDict(cells, book)
            walls.append((time.perf_counter() - t0) * 1e3)
    # the parts, once more by hand
    t0 = time.perf_counter()
    copies = D._Copies(cells, list(np.unique(book['chr'])))
    keys = {}
    from itertools import combinations_with_replacement
    for c1, c2 in combinations_with_replacement(np.unique(book['chr']), 2):
        keys.update(D._checked_keys(copies, c1, c2))
    host_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    pop = L.DistancePopulation.upload(copies.tables)
    up_ms = (time.perf_counter() - t0) * 1e3

    def all_keys():
        for key, pairs in keys.items():
            pop.summary(pairs[:, 0], pairs[:, 1], same=isinstance(key, str) and key.startswith("cis_"))

    calls_ms, k = timed(L, all_keys, a.runs)
    tiles = {}
    for tile in (4, 2):
        L.check(L.lib().ia3_set_tuning(L.IA3_TUNE_DIST_TILE, tile))
        w, kk = timed(L, all_keys, a.runs)
        tiles["tile%d" % tile] = dict(device_calls_wall_ms=w, kernel_ms=kk)
    L.check(L.lib().ia3_set_tuning(L.IA3_TUNE_DIST_TILE, 0))
    pop.free()
    gen = dict(gpu=gpu, chromosomes=len(chrs), regions=Rg, cells=cells_n, homologs=2, keys=len(out), copies=len(copies.tables),
               distances=int(sum(len(p) for p in keys.values())) * Rg * Rg, runs=a.runs,
               function_wall_ms=float(np.median(walls)), host_tables_and_pairs_ms=host_ms, upload_ms=up_ms,
               device_calls_wall_ms=calls_ms, kernel_ms=k, kernel_share_of_device_calls=sum(k.values()) / calls_ms, forced_tiles=tiles)
    print(json.dumps(gen), flush=True)
    merge(a.out, "genome_set", gen)


if __name__ == "__main__":
    main()
