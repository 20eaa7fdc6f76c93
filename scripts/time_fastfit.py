"""Wall time of the Fitting_v4 fast path next to fit_fov_image on the same seeds (needs a GPU).

    python scripts/time_fastfit.py [Z X Y n_spots] [--repeat K]

Seeds come from get_seeds on a synthetic field of view that is uploaded once; fast_fit_big_image (moment fits, with
and without the Voronoi test and the re-centring) and fit_fov_image(seeds=...) (LM first fits and refit sweeps) then
run on those seeds.  get_seed_points_base_v2 is timed on the same stack.  Prints one JSON line with the median of the
repeats per entry; read it with the rules of DESIGN.md §5 (warm-up, medians, a quiet machine).
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def median_ms(fn, repeat):
    fn()                                    # warm-up: scratch buffers, code objects
    ts = []
    for _ in range(repeat):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts))


def main():
    from imageanalysis3_amd import _lib as L, synth
    from imageanalysis3_amd.External.Fitting_v4 import fast_fit_big_image, get_seed_points_base_v2
    from imageanalysis3_amd.spot_tools.fitting import fit_fov_image, get_seeds
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    repeat = int(sys.argv[sys.argv.index("--repeat") + 1]) if "--repeat" in sys.argv else 5
    Z, X, Y, n = (int(v) for v in args[:4]) if len(args) >= 4 else (30, 1024, 1024, 2000)
    L.check(L.lib().ia3_init(0))
    im, _, _ = synth.make_fov((Z, X, Y), n, 1)
    seeds = get_seeds(im, th_seed=600)
    out = {"shape": [Z, X, Y], "seeds": int(len(seeds)), "repeat": repeat}
    with L.DeviceStack.upload(im) as stack:
        out["moments_ms"] = median_ms(lambda: fast_fit_big_image(stack, seeds), repeat)
        out["moments_recenter_ms"] = median_ms(lambda: fast_fit_big_image(stack, seeds, recenter=True), repeat)
        out["moments_no_voronoi_ms"] = median_ms(lambda: fast_fit_big_image(stack, seeds, avoid_neigbors=False), repeat)
        out["seeds_v2_ms"] = median_ms(lambda: get_seed_points_base_v2(stack, gfilt_size=5, th_seed=6.), repeat)
    out["fit_fov_image_ms"] = median_ms(lambda: fit_fov_image(im, "647", seeds=seeds, verbose=False), repeat)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
