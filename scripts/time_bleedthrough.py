"""Times the tail of the bleedthrough-profile generator on the device (ia3_bleedthrough_profile_dev, csrc/calib.hip)
and its NumPy restatement.

    python scripts/time_bleedthrough.py [--depths 30 50] [--size 2048] [--runs 15] [--no-cpu] [--out profiles/bleedthrough.json]

(i)  the kernel at (depth, size, size), C = 3, fitting order 2, float64, with and without the mean over z, inverting:
     the kernel's HIP-event time (ia3_profile_collect) and the host wall time of the call with its allocation, warm,
     median over the runs; next to them the two yardsticks: the time the output alone takes at 8 TB/s, and the number of
     unfused float64 operations per pixel, about depth * (6 + 6 * 19) for the polynomials;
(ii) the NumPy restatement of the same tail (np.indices -> generate_polynomial_data -> np.dot for six directions, the
     stack, the mean over z, np.linalg.inv per pixel from a Python loop, as bleedthrough.py:451-486 does) on a
     256 x 256 tile on this machine's CPU, scaled by area to the full size and labelled as scaled.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from imageanalysis3_amd import _lib as L                                              # noqa: E402
from imageanalysis3_amd.correction_tools.chromatic import generate_polynomial_data    # noqa: E402
from harness import bleed_ref as B                                                    # noqa: E402
from time_chromatic import stage_times                                                # noqa: E402

ROOFLINE_TBPS = 8.0
TILE = 256


def numpy_tail(consts, present, order, center, shape, mean_z):
    """The reference's tail, restated: returns the inverse profile."""
    n_ch = consts.shape[0]
    grid = np.indices(shape).reshape(3, -1) - np.asarray(center)[:, np.newaxis]
    prof = np.zeros((n_ch, n_ch) + tuple(shape))
    for r in range(n_ch):
        for t in range(n_ch):
            if r == t:
                prof[t, r] = np.ones(shape)
            elif present[t, r]:
                pX = generate_polynomial_data(grid.transpose(), order)     # once per direction, as the reference
                prof[t, r] = np.dot(pX, consts[t, r]).reshape(shape)
    if mean_z:
        prof = prof.mean(2)
    out = np.zeros(np.shape(prof), dtype=float)
    for i in range(prof.shape[-2]):
        for j in range(prof.shape[-1]):
            if mean_z:
                out[:, :, i, j] = np.linalg.inv(prof[:, :, i, j])
            else:
                for z in range(prof.shape[-3]):
                    out[:, :, z, i, j] = np.linalg.inv(prof[:, :, z, i, j])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--depths", type=int, nargs="+", default=[30, 50])
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bleedthrough.json"))
    a = ap.parse_args()
    L.check(L.lib().ia3_init(0))
    name = C.create_string_buffer(256)
    L.lib().ia3_device_name(name, 256)
    order, n_ch = 2, 3
    consts, present = B.tail_constants(n_ch, order, 1)
    consts = consts * (50.0 / (a.size / 2)) ** 2          # the polynomials stay below 0.3 over the larger field
    res = dict(size=a.size, runs=a.runs, channels=n_ch, fitting_order=order, dtype="float64",
               gpu=name.value.decode(), kernel={})

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")

    for depth in a.depths:
        shape = (depth, a.size, a.size)
        center = np.array(shape) / 2
        for mean_z in (True, False):
            def call():
                L.lib().ia3_buffer_free(L.bleedthrough_profile(consts, present, order, center, shape, mean_z=mean_z,
                                                               invert=True, dtype=np.float64))
            s, w = stage_times(call, a.runs)
            nbytes = n_ch * n_ch * (1 if mean_z else depth) * a.size * a.size * 8
            res["kernel"]["z%d_%s" % (depth, "mean_z" if mean_z else "per_z")] = dict(
                kernel_ms=s.get("bleed_profile"), call_wall_ms=w, output_bytes=nbytes,
                store_at_roofline_ms=nbytes / (ROOFLINE_TBPS * 1e12) * 1e3,
                f64_operations_per_output_matrix=depth * (6 + 6 * 19) if mean_z else 6 + 6 * 19,
                f64_operations_per_s=depth * (6 + 6 * 19) * a.size * a.size / (s["bleed_profile"] * 1e-3))
            print(json.dumps(res["kernel"]), flush=True)
            write()

    if not a.no_cpu:
        res["cpu_numpy_scaled"] = {}
        scale = (a.size / TILE) ** 2
        for depth in a.depths:
            shape = (depth, TILE, TILE)
            center = np.array([depth, a.size, a.size]) / 2
            for mean_z in (True, False):
                t0 = time.perf_counter()
                numpy_tail(consts, present, order, center, shape, mean_z)
                t = time.perf_counter() - t0
                res["cpu_numpy_scaled"]["z%d_%s" % (depth, "mean_z" if mean_z else "per_z")] = dict(
                    tile=[depth, TILE, TILE], tile_s=t, scaled_by_area=scale, scaled_s=t * scale)
                print(json.dumps(res["cpu_numpy_scaled"]), flush=True)
                write()


if __name__ == "__main__":
    main()
