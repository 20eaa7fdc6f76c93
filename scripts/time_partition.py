"""Wall time of the label kernels and of the per-cell route next to the flat replay (needs a GPU).

    python scripts/time_partition.py [Z X Y n_spots cells_per_side] [--repeat K] [--no-replay]

A synthetic field of view (imageanalysis3_amd/synth.py) and a label image of cells_per_side^2 ellipsoidal cells on a
grid.  Timed: ``ia3_label_boxes_dev`` on the resident label stack; the vote (radius 10), the maximum (radius 5) and the
gather (radius 3) around every seed of the field; ``fit_spots_by_segmentation`` with everything resident; and, unless
``--no-replay``, ``tests/harness/replay.py::fit_in_labels`` on the same stacks, which builds one mask per cell over the
whole label image on the host as the reference does (minutes on a full-size field: start small).  The two routes'
tables are compared bit for bit.  Prints one JSON line with the median of the repeats per entry; read it with the rules
of DESIGN.md §5 (warm-up, medians, a quiet machine).  Nothing here has been measured yet: DESIGN.md §18 states no figure.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def median_ms(fn, repeat):
    fn()                                    # warm-up: scratch buffers, code objects
    ts = []
    for _ in range(repeat):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts))


def grid_cells(shape, per_side):
    """uint16 label image: per_side x per_side ellipsoids, each painted inside its own grid cell only."""
    Z, X, Y = shape
    lab = np.zeros(shape, np.uint16)
    sx, sy = X // per_side, Y // per_side
    z = (np.arange(Z) - Z / 2.) / (Z / 2.2)
    x = (np.arange(sx) - sx / 2.) / (sx / 2.3)
    y = (np.arange(sy) - sy / 2.) / (sy / 2.3)
    ell = (z[:, None, None] ** 2 + x[None, :, None] ** 2 + y[None, None, :] ** 2) <= 1
    for i in range(per_side):
        for j in range(per_side):
            lab[:, i * sx:(i + 1) * sx, j * sy:(j + 1) * sy][ell] = 1 + i * per_side + j
    return lab


def main():
    from imageanalysis3_amd import _lib as L, synth
    from imageanalysis3_amd.classes.preprocess import fit_spots_by_segmentation
    from imageanalysis3_amd.spot_tools.fitting import get_seeds
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    repeat = int(sys.argv[sys.argv.index("--repeat") + 1]) if "--repeat" in sys.argv else 5
    if "--repeat" in sys.argv:
        args.remove(sys.argv[sys.argv.index("--repeat") + 1])
    Z, X, Y, n, side = (int(v) for v in args[:5]) if len(args) >= 5 else (30, 512, 512, 800, 6)
    L.check(L.lib().ia3_init(0))
    im, _, _ = synth.make_fov((Z, X, Y), n, 1)
    lab = grid_cells((Z, X, Y), side)
    seeds = get_seeds(im, th_seed=600)
    out = {"shape": [Z, X, Y], "cells": side * side, "seeds": int(len(seeds)), "repeat": repeat}
    with L.DeviceStack.upload(im) as stack, L.DeviceStack.upload(lab) as labels:
        out["label_boxes_ms"] = median_ms(lambda: L.label_boxes(labels, 65535), repeat)
        out["vote_r10_ms"] = median_ms(lambda: L.cube_labels(labels, seeds, 10), repeat)
        out["max_r5_ms"] = median_ms(lambda: L.cube_max(stack, seeds, 5), repeat)
        out["gather_r3_ms"] = median_ms(lambda: L.cube_gather(stack, seeds, 3), repeat)
        run = lambda: fit_spots_by_segmentation(stack, "647", labels, th_seed=600)   # noqa: E731
        out["fit_by_segmentation_ms"] = median_ms(run, repeat)
        spots, ids = run()
        out["kept_spots"] = int(len(spots))
        if "--no-replay" not in sys.argv:
            from harness import replay as R
            L.check(L.lib().ia3_set_tuning(L.IA3_TUNE_COL_RTC, 0))   # as on the other side: time no run-time compile
            try:
                t = time.perf_counter()
                want, want_ids = R.fit_in_labels(stack, "647", lab, np.zeros(3), th_seed=600)
                out["replay_ms"] = (time.perf_counter() - t) * 1e3   # (one run: it is the slow side)
            finally:
                L.check(L.lib().ia3_set_tuning(L.IA3_TUNE_COL_RTC, 1))
            out["equal_bits"] = bool(np.asarray(spots).tobytes() == np.asarray(want).tobytes()
                                     and np.asarray(ids).tobytes() == np.asarray(want_ids).tobytes())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
