"""Times find_candidate_chromosomes and its stages on a resident stack.

    python scripts/time_chromosome.py [--shape 50 2048 2048] [--dtype u16] [--runs 10] [--no-cpu] [--out profiles/chromosome.json]

(i)   the fused entry (ia3_find_candidate_chromosomes_dev) on a resident synthetic stack: per-stage HIP-event times
      (ia3_profile_collect: the select passes, range filter, mask, erosions / dilations, labelling, hole filling, sums),
      warm, median over the runs, and the host wall time of the call;
(ii)  every operator alone on resident masks: plane medians, seed mask, erosion, dilation, closing, hole filling, label,
      label centres, small-label removal (host wall time around a synchronised call, warm, median);
(iii) the host statement of the same chain (tests/harness/chromseg_ref.py) on a smaller stack, one run.
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

from imageanalysis3_amd import _lib as L                                              # noqa: E402
from imageanalysis3_amd.segmentation_tools import morphology as M                     # noqa: E402


def med(v):
    return float(np.median(np.asarray(v, dtype=np.float64)))


def stage_times(fn, runs, warm=2):
    """{stage: median ms} from ia3_profile_collect over `runs` calls of fn, and the median host wall time (ms)."""
    for _ in range(warm):
        fn()
    L.check(L.lib().ia3_sync())
    L.profile_enable(True)
    L.profile_collect()
    per, wall = {}, []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        L.check(L.lib().ia3_sync())
        wall.append((time.perf_counter() - t0) * 1e3)
        for k, (n, ms) in L.profile_collect().items():
            per.setdefault(k, []).append(ms)
    L.profile_enable(False)
    return {k: med(v) for k, v in per.items()}, med(wall)


def synthetic(shape, dtype, seed=5):
    """Poisson(400) background with one blob per ~2 M voxels, built plane group by plane group."""
    from harness import chromseg_cases as CC
    Z, X, Y = shape
    tz, tx, ty = min(Z, 25), min(X, 256), min(Y, 256)
    tile = CC.stack((tz, tx, ty), 4, seed, dtype)
    reps = [int(np.ceil(s / float(t))) for s, t in zip(shape, tile.shape)]
    return np.ascontiguousarray(np.tile(tile, reps)[:Z, :X, :Y])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=[50, 2048, 2048])
    ap.add_argument("--dtype", choices=("u16", "f32"), default="u16")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--filt-size", type=int, default=4)
    ap.add_argument("--per", type=float, default=99.5)
    ap.add_argument("--min-size", type=int, default=100)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--cpu-shape", type=int, nargs=3, default=[25, 256, 256])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chromosome.json"))
    a = ap.parse_args()
    shape = tuple(a.shape)
    L.check(L.lib().ia3_init(0))
    name = C.create_string_buffer(256)
    L.lib().ia3_device_name(name, 256)
    res = dict(shape=list(shape), dtype=a.dtype, runs=a.runs, filt_size=a.filt_size, per=a.per, min_size=a.min_size,
               gpu=name.value.decode())
    im = synthetic(shape, a.dtype)

    def wall(fn):
        return stage_times(fn, a.runs)[1]

    with L.DeviceStack.upload(im) as st:
        # (i) the fused entry
        coords, th, _ = L.find_candidate_chromosomes(st, a.filt_size, a.per, 1, a.min_size)
        stages, w = stage_times(lambda: L.find_candidate_chromosomes(st, a.filt_size, a.per, 1, a.min_size), a.runs)
        res["fused"] = dict(call_wall_ms=w, stages_ms=stages, stage_sum_ms=sum(stages.values()), objects=int(len(coords)),
                            threshold=float(th))
        print(json.dumps(res["fused"]), flush=True)
        # (ii) the operators alone
        ops = {}
        ops["plane_medians_ms"] = wall(lambda: L.plane_medians(st))
        ops["seed_mask_ms"] = wall(lambda: L.chrom_seed_mask(st, a.filt_size, a.per)[0].free())
        mask, _ = L.chrom_seed_mask(st, a.filt_size, a.per)
        with mask:
            ops["erosion_ball1_ms"] = wall(lambda: L.binary_morph(mask, L.MORPH_ERODE, 1).free())
            ops["dilation_ball1_ms"] = wall(lambda: L.binary_morph(mask, L.MORPH_DILATE, 1).free())
            ops["dilation_ball2_ms"] = wall(lambda: L.binary_morph(mask, L.MORPH_DILATE, 2).free())
            ops["closing_ball1_ms"] = wall(lambda: L.binary_morph(mask, L.MORPH_CLOSE, 1).free())
            ops["fill_holes_ms"] = wall(lambda: L.binary_fill_holes(mask).free())
            ops["label_ms"] = wall(lambda: L.label(mask).free())
            with L.label(mask) as lab:
                ops["components"] = lab.n
                ops["label_centers_ms"] = wall(lambda: L.label_centers(lab, lab.n))
                ops["remove_small_ms"] = wall(lambda: L.remove_small_labels(lab, lab.n, a.min_size).free())
        res["operators"] = ops
        print(json.dumps(ops), flush=True)

    # (iii) the host statement on a smaller stack
    if not a.no_cpu:
        from harness import chromseg_ref as R
        small = synthetic(tuple(a.cpu_shape), a.dtype)
        t0 = time.perf_counter()
        st_ref = R.chain(small, a.filt_size, a.per, 1, a.min_size)
        t1 = time.perf_counter()
        with L.DeviceStack.upload(small) as ds:
            got, _, _ = L.find_candidate_chromosomes(ds, a.filt_size, a.per, 1, a.min_size)
            _, w_small = stage_times(lambda: L.find_candidate_chromosomes(ds, a.filt_size, a.per, 1, a.min_size), a.runs)
        res["cpu_statement"] = dict(shape=list(a.cpu_shape), chain_s=t1 - t0, device_call_wall_ms=w_small,
                                    objects=int(len(st_ref["ids"])),
                                    equal_to_device=bool(got.tobytes() == np.asarray(st_ref["coords"], dtype=np.float64).tobytes()))
        print(json.dumps(res["cpu_statement"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
