"""Times chromosome selection by candidate spots (csrc/select.hip) on an experiment-sized input.

    python scripts/time_select_chromosomes.py [--rounds 500] [--spots 4000] [--candidates 400] [--runs 5] [--check]
                                              [--out profiles/select_chromosomes.json]
    python scripts/time_select_chromosomes.py --cpu-literal [--max-passes N]

The workload: `--rounds` rounds of `--spots` selected spots each around `--candidates` candidate centres, a quarter of
which show a spot in three rounds of ten (absent from more than 40 % of the rounds); default thresholds.

Without --cpu-literal (needs the GPU): the library call ia3_select_chromosomes_dev, warm, median over the runs, with the
host clock the library takes around its three parts, each ended by a synchronise: the upload, the first pass (every spot
against every candidate) and the removal loop (number of removals and mean per removal); the wall time of the library
call and of the whole public call (select_candidate_chromosomes, with the host's selection and scaling of the rows); the
candidates visited against the bound S C + sum m_k a_k.  --check holds the result against the statement's incremental form.

With --cpu-literal (no GPU): the statement's literal loop (tests/harness/select_ref.py), which is the reference's
algorithm, on the same input on this host's CPU; it runs for minutes (--max-passes stops it early and says so).  Both
parts write into the same JSON file.
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

VOLUME = (50, 2048, 2048)


def workload(n_rounds, per_round, n_cand, seed=11):
    """(cands (C, 3) float64 pixels, list of (per_round, 5) float32 spot tables [intensity, z, x, y, row id])."""
    rs = np.random.RandomState(seed)
    cands = rs.uniform(0, 1, (n_cand, 3)) * np.array(VOLUME)
    p = np.full(n_cand, 0.95)
    p[rs.permutation(n_cand)[:n_cand // 4]] = 0.3
    spots_list = []
    for r in range(n_rounds):
        present = np.flatnonzero(rs.rand(n_cand) < p)
        who = np.concatenate([present, present[rs.randint(0, len(present), max(0, per_round - len(present)))]])[:per_round]
        t = np.empty((per_round, 5), dtype=np.float32)
        t[:, 0] = rs.uniform(0.5, 4.0, per_round)
        t[:, 1:4] = cands[who] + rs.normal(0, 1, (per_round, 3)) * np.array([1.0, 3.0, 3.0])
        t[:, 4] = np.arange(per_round)
        spots_list.append(t)
    return cands, spots_list


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
    ap.add_argument("--rounds", type=int, default=500)
    ap.add_argument("--spots", type=int, default=4000)
    ap.add_argument("--candidates", type=int, default=400)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--cpu-literal", action="store_true")
    ap.add_argument("--max-passes", type=int, default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "select_chromosomes.json"))
    a = ap.parse_args()
    cands, spots_list = workload(a.rounds, a.spots, a.candidates)
    shape = dict(rounds=a.rounds, spots_per_round=a.spots, candidates=a.candidates, intensity_th=0.5, loss_th=0.4)
    from harness import select_ref as R
    if a.cpu_literal:
        t0 = time.perf_counter()
        rec = R.literal(cands, spots_list, max_passes=a.max_passes)
        dt = time.perf_counter() - t0
        out = dict(shape, seconds=dt, removals=int(len(rec["removed"])), kept=int(len(rec["kept"])), visits=rec["visits"],
                   complete=a.max_passes is None, cpus=os.cpu_count())
        print(json.dumps(out), flush=True)
        merge(a.out, "numpy_literal_loop", out)
        return
    from imageanalysis3_amd import _distance_zxy, _lib as L
    from imageanalysis3_amd.segmentation_tools import chromosome as CH
    L.check(L.lib().ia3_init(0))
    name = C.create_string_buffer(256)
    L.lib().ia3_device_name(name, 256)
    t0 = time.perf_counter()
    _, zxys, starts = CH._pack_rounds(spots_list, 0.5, _distance_zxy)
    chrom = np.array(list(cands)) * np.array(_distance_zxy)
    pack_ms = (time.perf_counter() - t0) * 1e3
    L.select_chromosomes(zxys, starts, chrom, 0.4)                                    # warm
    parts, walls, full = [], [], []
    for _ in range(a.runs):
        t0 = time.perf_counter()
        res = L.select_chromosomes(zxys, starts, chrom, 0.4, times=True)
        walls.append((time.perf_counter() - t0) * 1e3)
        parts.append(res["times_ms"])
        t0 = time.perf_counter()
        kept = CH.select_candidate_chromosomes(cands, spots_list, _verbose=False)
        full.append((time.perf_counter() - t0) * 1e3)
    up, first, loop = np.median(np.array(parts), axis=0)
    n_rem = int(len(res["removed"]))
    S, C = len(zxys), len(chrom)
    out = dict(shape, gpu=name.value.decode(), runs=a.runs, selected_spots=S, upload_ms=float(up),
               upload_bytes=int(zxys.nbytes + chrom.nbytes + starts.nbytes), first_pass_ms=float(first),
               first_pass_distances=S * C, removal_loop_ms=float(loop), removals=n_rem, kept=int(len(kept)),
               removal_mean_ms=float(loop / n_rem) if n_rem else None, library_call_wall_ms=float(np.median(walls)),
               public_call_wall_ms=float(np.median(full)), host_select_and_scale_ms=pack_ms, visits=res["visits"],
               visits_if_every_pass_were_whole=int(S * sum(C - k for k in range(n_rem + 1))))
    if a.check:
        rec = R.incremental(cands, spots_list)
        out["equal_to_statement"] = bool(np.array_equal(res["removed"], rec["removed"]) and res["visits"] == rec["visits"] and
                                         np.array_equal(res["lost"], rec["lost"]) and kept.tobytes() == rec["coords"].tobytes())
    print(json.dumps(out), flush=True)
    merge(a.out, "device", out)


if __name__ == "__main__":
    main()
