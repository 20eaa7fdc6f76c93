"""Times the population picker (csrc/pick.hip) on an experiment-sized population.

    python scripts/time_pick_spots.py [--chromosomes 2000] [--regions 1000] [--iterations 5] [--runs 3] [--check]
                                      [--out profiles/pick_spots.json]
    python scripts/time_pick_spots.py --cpu-statement [--fraction 20]

The workload: `--chromosomes` random-walk chromosomes of `--regions` regions with 1-6 candidates per region, three channels
interleaved and split both ways, windows of 7 ids, `--iterations` EM iterations from the brightest candidates.

Without --cpu-statement (needs the GPU): the upload once, then the loop on the resident population, warm, median over the
runs.  HIP events on the library stream per stage (E-step with its centres, the radix sorts, M-step with its centres, the
difference), summed over the iterations, the wall time of the whole loop (``em_pick_spots`` on the handle: kernels, the
host's window tables, the 8-byte reads) and what crossed PCIe per iteration (the log tables go up only when the length
of a reference array changes).  --check holds the first iteration of
a 1/100 population against the statement (tests/harness/pick_ref.py) bit for bit.

With --cpu-statement (no GPU): the statement, which is the reference's arithmetic in NumPy, for ONE iteration on 1/`--fraction`
of the chromosomes on one CPU core.  Both parts write into the same JSON file.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

CHANNELS = ["750", "647", "561"]
NEIGHBOR_LEN = 7


def workload(P, R, seed=21):
    """Ragged ``cands[p][r]``: (k, 4) tables of h, z, x, y in nm, k = 1..6; the first row of each lies near the walk."""
    rs = np.random.RandomState(seed)
    cands = []
    for p in range(P):
        walk = rs.uniform(2000, 40000, 3) + np.cumsum(rs.normal(0, 300, (R, 3)), axis=0)
        k = rs.randint(1, 7, R)
        n = int(k.sum())
        t = np.empty((n, 4))
        first = np.concatenate([[0], np.cumsum(k)[:-1]])
        owner = np.repeat(np.arange(R), k)
        t[:, 0] = 1 + 0.25 * rs.randint(0, 24, n)
        t[:, 1:] = walk[owner] + rs.uniform(-1500, 1500, (n, 3))
        t[first, 0] += 3
        t[first, 1:] = walk + rs.normal(0, 60, (R, 3))
        cands.append(np.split(t, first[1:]))
    channels = [CHANNELS[j % 3] for j in range(R)]
    return cands, channels


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


def statement_iteration(R_, cands, channels):
    ids = list(range(len(channels)))
    picks0, _ = R_.pick_by_intensity(cands)
    e = R_.e_step(picks0, ids, picks0, ids, NEIGHBOR_LEN, channels, True, None)
    m = R_.m_step(cands, ids, picks0, ids, e["sorted"], NEIGHBOR_LEN, 1.0, 1.0, channels, True, True, None)
    return picks0, e, m, R_.difference(picks0, m["picks"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chromosomes", type=int, default=2000)
    ap.add_argument("--regions", type=int, default=1000)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--fraction", type=int, default=20)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--cpu-statement", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pick_spots.json"))
    a = ap.parse_args()
    from harness import pick_ref as R_
    P, R = a.chromosomes, a.regions
    shape = dict(chromosomes=P, regions=R, channels=3, neighbor_len=NEIGHBOR_LEN, iterations=a.iterations)
    if a.cpu_statement:
        sub = max(1, P // a.fraction)
        cands, channels = workload(sub, R)
        t0 = time.perf_counter()
        _, _, m, diff = statement_iteration(R_, cands, channels)
        dt = time.perf_counter() - t0
        out = dict(chromosomes=sub, regions=R, candidates=int(len(m["scores"])), iterations=1, seconds=dt, difference=list(diff),
                   threads=1)
        print(json.dumps(out), flush=True)
        merge(a.out, "numpy_statement_one_core", out)
        return
    from imageanalysis3_amd import _lib as L
    from imageanalysis3_amd.spot_tools import picking as PK
    L.check(L.lib().ia3_init(0))
    name = C.create_string_buffer(256)
    L.lib().ia3_device_name(name, 256)
    cands, channels = workload(P, R)
    t0 = time.perf_counter()
    packed = PK._pack(cands)
    pack_ms = (time.perf_counter() - t0) * 1e3
    pop = PK.upload_population(cands, None, None, channels)
    # the library call alone (allocation of the handle's tables and the copies), on the packed tables
    t0 = time.perf_counter()
    again = L.PickPopulation.upload(packed[0], packed[1], packed[2], P, R, PK._channel_codes(channels)[0], 3)
    upload_ms = (time.perf_counter() - t0) * 1e3
    again.free()
    kw = dict(n_iter_max=a.iterations, stop_ratio=2.0, neighbor_len=NEIGHBOR_LEN, split_intensity_channels=True,
              split_distance_channels=True)
    PK.em_pick_spots(pop, **kw)                                                          # warm
    walls, stages = [], []
    for _ in range(a.runs):
        L.profile_enable(True)
        L.profile_collect()
        t0 = time.perf_counter()
        picks, scores, ratios = PK.em_pick_spots(pop, **kw)
        walls.append((time.perf_counter() - t0) * 1e3)
        prof = L.profile_collect()
        L.profile_enable(False)
        stages.append({k: v[1] for k, v in prof.items() if k.startswith("pick_")})
    med = {k: float(np.median([s.get(k, 0.0) for s in stages])) for k in stages[0]}
    lens = pop.lengths.copy()
    log_bytes = int(sum(8 * len(t) for _, t in pop._logs.values()))
    ws, wi = PK._windows(pop.cand_ids, pop.ref_ids, NEIGHBOR_LEN, pop.ref_channels, True)
    out = dict(shape, gpu=name.value.decode(), runs=a.runs, candidates=int(pop.n),
               host_pack_ms=pack_ms, upload_ms=upload_ms, upload_bytes=int(packed[0].nbytes + packed[1].nbytes + packed[2].nbytes),
               stage_ms_over_all_iterations=med, stage_sum_ms=float(sum(med.values())),
               loop_wall_ms=float(np.median(walls)), ratios=[float(r) for r in ratios],
               reference_lengths_all=[int(v) for v in lens[:, pop.n_channels]],
               per_iteration_host_to_device_bytes=int(2 * (ws.nbytes + wi.nbytes)),
               log_table_bytes_when_a_length_changes=log_bytes,
               per_iteration_device_to_host_bytes=int(lens.nbytes + 8))
    if a.check:
        sub = max(1, P // 100)
        small, _ = workload(sub, R)
        picks0, e, m, diff = statement_iteration(R_, small, channels)
        p1, s1, r1 = PK.em_pick_spots(small, n_iter_max=1, stop_ratio=2.0, ref_channels=channels, neighbor_len=NEIGHBOR_LEN,
                                      split_intensity_channels=True, split_distance_channels=True)
        out["equal_to_statement"] = bool(R_.same_bits(p1, m["picks"]) and R_.same_bits(s1, m["sel_scores"]) and
                                         r1[0] == np.int64(diff[0]) / np.int64(diff[1]))
    pop.free()
    print(json.dumps(out), flush=True)
    merge(a.out, "device", out)


if __name__ == "__main__":
    main()
