"""Wall time of the views of a fit (gparms, ims_rec, im_subtr / im_add, residual_stack) on the bench field of view
(needs a GPU).

    python scripts/time_fit_views.py [Z X Y n_spots] [--repeat K]

Default: the bench FOV, 50 x 2048 x 2048 float32 with 5 000 spots, uploaded once, seeded with th_seed 600 and fitted
(firstfit + repeatfit) before anything is timed.  Every entry is the median of K runs after one warm-up run, with the
library stream drained before the clock starts and before it stops.  The entries that return host arrays
include their device-to-host copy, which for the float64 residual is the whole volume — 8 bytes a voxel, 1.68 GB for the
bench FOV: `residual_f64_device_ms` is the render alone (the entry called without a host buffer), and
`residual_f64_download_ms` the rest of the call that fills one.  None of this is on the per-FOV path.  Prints one JSON
line.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def median_ms(fn, repeat, sync):
    fn()                                    # warm-up: scratch buffers, code objects
    ts = []
    for _ in range(repeat):
        sync()
        t = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts))


def main():
    from imageanalysis3_amd import _lib as L, synth
    from imageanalysis3_amd.External.Fitting_v4 import iter_fit_seed_points
    from imageanalysis3_amd.spot_tools.fitting import get_seeds
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    repeat = int(sys.argv[sys.argv.index("--repeat") + 1]) if "--repeat" in sys.argv else 7
    Z, X, Y, n = (int(v) for v in args[:4]) if len(args) >= 4 else (50, 2048, 2048, 5000)
    lib = L.lib()
    L.check(lib.ia3_init(0))

    def sync():
        L.check(lib.ia3_sync())

    im, _, _ = synth.make_fov((Z, X, Y), n, 1)
    out = {"shape": [Z, X, Y], "repeat": repeat}
    with L.DeviceStack.upload(im) as stack:
        seeds = get_seeds(stack, th_seed=600)
        f = iter_fit_seed_points(stack, seeds.T)
        f.firstfit()
        f.repeatfit()
        out["seeds"], out["n_iter"] = int(len(seeds)), int(f.n_iter)
        h = f._fitter
        out["snapshot_ms"] = median_ms(lambda: L.check(lib.ia3_fit_snapshot(h)), repeat, sync)
        # (taken again after repeatfit() the snapshot holds the final records: the same copy, and im_subtr below then
        # costs what im_add costs)
        out["voxel_sets_ms"] = median_ms(f._render_gparms, repeat, sync)
        out["reconstructions_ms"] = median_ms(f._render_ims_rec, repeat, sync)
        out["residual_f32_stack_ms"] = median_ms(lambda: f.residual_stack("add").free(), repeat, sync)
        out["residual_f64_device_ms"] = median_ms(lambda: L.check(lib.ia3_fit_view_residual(h, 1, None)), repeat, sync)
        host = np.empty((Z, X, Y), dtype=np.float64)
        total = median_ms(lambda: L.check(lib.ia3_fit_view_residual(h, 1, L.dptr(host))), repeat, sync)
        out["residual_f64_download_ms"] = total - out["residual_f64_device_ms"]
        out["residual_f64_bytes"] = int(host.nbytes)
        f.release()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
