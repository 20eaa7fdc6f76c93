"""Times the chromosomal spot scores (csrc/score.hip) on an experiment-sized workload.

    python scripts/time_scoring.py [--chromosomes 2000] [--runs 3] [--out profiles/scoring.json]
    python scripts/time_scoring.py --cpu-reference [--fraction 100]

The workload: `--chromosomes` traced chromosomes of 1000 regions with 5 candidate spots per region (a Gaussian walk, 5 % of
the selected spots NaN) and one selected spot per region, scored with chromosomal_spot_scores' defaults in both metrics
('cdf' against cdf references, 'linear' against median references).

Without --cpu-reference (needs the GPU): one upload, then per metric the median over the runs of the wall time of the call
(host glue with np.log, library call, download) and of the HIP-event times of its kernels, and the same for
replace_selected followed by rescoring.  The first chromosome is held against the NumPy statement below bit for bit.

With --cpu-reference (no GPU): the reference's procedure restated in NumPy (a Python loop per spot around np.where,
np.nanmean and np.nanmedian, a `data <= v` scan per spot and score) on one core for `--chromosomes` / `--fraction`
chromosomes.  Both parts write into the same JSON file.
"""
import argparse
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

R, PER, TH = 1000, 5, 1.
DZXY = np.array([200., 108., 108.])


def make_chromosomes(n, seed=0):
    rs = np.random.RandomState(seed)
    cands, ids, sels = [], [], []
    for _ in range(n):
        walk = np.cumsum(rs.normal(0, 1., (R, 3)), axis=0) + np.array([15., 1000., 1000.])
        c = np.repeat(walk, PER, axis=0) + rs.normal(0, 1.5, (R * PER, 3))
        cands.append(np.concatenate([np.exp(rs.normal(1., 1., (R * PER, 1))), c], axis=1))
        ids.append(np.repeat(np.arange(R), PER))
        s = np.concatenate([np.exp(rs.normal(1.5, 1., (R, 1))), walk + rs.normal(0, 0.5, (R, 3))], axis=1)
        s[rs.rand(R) < 0.05, 1:] = np.nan
        sels.append(s)
    return cands, ids, sels


# ---- the reference's procedure in NumPy ------------------------------------------------------------------------------------------

def np_local(zxys, ids, sel_zxys, sel_ids, local_size=5):
    half = int((local_size - 1) / 2)
    out = []
    for zxy, i in zip(zxys, ids):
        rows = [sel_zxys[k] for j in range(i - half, i + half + 1) if j != i for k in np.where(sel_ids == j)[0]]
        rows = np.array(rows)
        if len(rows) == 0 or (np.isnan(rows).sum(1) > 0).all():
            out.append(np.nan)
        else:
            out.append(np.linalg.norm(np.nanmean(rows, axis=0) - zxy))
    return np.array(out)


def np_neighbors(zxys, ids):
    fwd, rev = [], []
    for zxy, i in zip(zxys, ids):
        if i + 1 in ids:
            fwd.append(np.nanmedian(np.linalg.norm(zxys[np.where(ids == i + 1)[0]] - zxy, axis=1)))
            rev.append(np.nanmedian(np.linalg.norm(zxys[np.where(ids == i - 1)[0]] - zxy, axis=1)))
        else:
            fwd.append(np.nan)
            rev.append(np.nan)
    return np.array(fwd), np.array(rev)


def np_cum_prob(data, x, vmin=-np.inf, vmax=np.inf):
    data = data[~np.isnan(data)]
    x = np.where(np.isnan(x), np.inf, x)
    p = np.array([np.sum(data <= v) / len(data) for v in x])
    lo, hi = np.sum(data <= vmin) / len(data), np.sum(data <= vmax) / len(data)
    p = p - lo if hi <= lo else (p - lo) / (hi - lo)
    p[p <= 0] = 0
    p[p >= 1] = 1
    return p


def np_scores(cand, ids, sel, metric):
    """chromosomal_spot_scores(cand, ids, sel, score_metric=metric or median references, intensity_th=TH) -> four vectors."""
    z, sz, sid = cand[:, 1:4] * DZXY, sel[:, 1:4] * DZXY, np.arange(len(sel))
    center = np.nanmean(sz, axis=0)
    refs = [np.linalg.norm(sz - center, axis=1), np_local(sz, sid, sz, sid), np_neighbors(sz, sid)[0], np.where(sel[:, 0] <= TH, np.nan, sel[:, 0])]
    refs = [r[~np.isnan(r)] for r in refs]
    fwd, rev = np_neighbors(z, ids)
    dists = [np.linalg.norm(z - center, axis=1), np_local(z, ids, sz, sid), np.nanmean([fwd, rev], axis=0)]
    out = []
    for d, r in zip(dists, refs[:3]):
        if metric == 'cdf':
            cdf = 1 - np_cum_prob(r, d, 0, np.inf)
            s = np.zeros(len(d))
            s[cdf > 0] = np.log(cdf[cdf > 0]) * 1.
            s[cdf <= 0] = -np.inf
        else:
            s = -1 * 1. * (d / np.nanmedian(r))
        s[np.isnan(d)] = -1000
        out.append(s)
    h = cand[:, 0]
    s = np.zeros(len(h))
    if metric == 'cdf':
        cdf = np_cum_prob(refs[3], h, TH)
        s[cdf > 0] = np.log(cdf[cdf > 0]) * 1.
        s[cdf <= 0] = -np.inf
    else:
        s[h <= 0] = -np.inf
        s[h > 0] = np.log(h[h > 0] / (h[h > 0] + np.nanmedian(refs[3]))) * 1.
    s[np.isnan(s)] = -1000
    s[np.isinf(s)] = -1000
    return out + [s]


def gpu_scores(pop, S, L, metric):
    if metric == 'cdf':
        return S.population_chromosomal_spot_scores(pop, 'cdf', intensity_th=TH)
    val, cls, _ = pop.scores('linear', 'median', 5, TH, True, (1., 1., 1., 1.), [0, np.inf])
    out = []
    for a in range(4):
        s = S._finish(val[a], cls[a], 1., val[a].shape)
        if a < 3:
            s[(cls[a] & L.SCORE_NAN_IN) != 0] = -1000
        else:
            s[np.isnan(s)] = -1000
            s[np.isinf(s)] = -1000
        out.append(s)
    return [tuple(s[pop.cand_start[c]:pop.cand_start[c + 1]] for s in out) for c in range(pop.C)]


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
    ap.add_argument("--chromosomes", type=int, default=2000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--fraction", type=int, default=100)
    ap.add_argument("--cpu-reference", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scoring.json"))
    a = ap.parse_args()
    warnings.filterwarnings("ignore")
    from harness import scoring_cases as K
    if a.cpu_reference:
        n = max(1, a.chromosomes // a.fraction)
        cands, ids, sels = make_chromosomes(n)
        res = dict(chromosomes=n)
        for metric in ('cdf', 'linear'):
            t0 = time.perf_counter()
            for c in range(n):
                np_scores(cands[c], ids[c], sels[c], metric)
            res[metric + "_s"] = time.perf_counter() - t0
        print(json.dumps(res))
        merge(a.out, "numpy_one_core", res)
        return
    from imageanalysis3_amd import _lib as L
    from imageanalysis3_amd.spot_tools import scoring as S
    L.check(L.lib().ia3_init(0))
    cands, ids, sels = make_chromosomes(a.chromosomes)
    t0 = time.perf_counter()
    pop = L.ScorePopulation.upload(cands, ids, sels, None, None, DZXY)
    t_upload = time.perf_counter() - t0
    res = dict(chromosomes=a.chromosomes, regions=R, candidates_per_region=PER, candidates=pop.N, selected=pop.S, upload_s=t_upload)
    kernels = ("score_geom", "score_refs", "score_values")
    for metric in ('cdf', 'linear'):
        first = gpu_scores(pop, S, L, metric)[0]                 # warm
        want = np_scores(cands[0], ids[0], sels[0], metric)
        assert all(K.same(g, w) for g, w in zip(first, want)), metric
        walls, ktimes = [], []
        for _ in range(a.runs):
            L.profile_enable(True)
            L.profile_collect()
            t0 = time.perf_counter()
            gpu_scores(pop, S, L, metric)
            walls.append(time.perf_counter() - t0)
            prof = L.profile_collect()
            ktimes.append(sum(prof[k][1] for k in kernels if k in prof) * 1e-3)
            L.profile_enable(False)
        res[metric + "_wall_s"], res[metric + "_kernel_s"] = float(np.median(walls)), float(np.median(ktimes))
    walls = []
    for r in range(a.runs):
        new = [np.roll(s, r + 1, axis=0) for s in sels]
        t0 = time.perf_counter()
        pop.replace_selected(new)
        gpu_scores(pop, S, L, 'cdf')
        walls.append(time.perf_counter() - t0)
    res["replace_and_rescore_wall_s"] = float(np.median(walls))
    pop.free()
    print(json.dumps(res))
    merge(a.out, "mi355x", res)


if __name__ == "__main__":
    main()
