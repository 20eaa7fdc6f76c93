"""Times the two device stages of the chromatic-profile generator (csrc/calib.hip) and their NumPy restatement.

    python scripts/time_chromatic.py [--shape 50 2048 2048] [--pairs 300] [--runs 15] [--no-cpu] [--out profiles/chromatic.json]

(i)   ia3_crop_pairs_dev: `--pairs` pairs of 9^3 boxes with their regressions on two resident uint16 stacks: the kernel's
      HIP-event time (ia3_profile_collect) and the host wall time of the call (uploads of the centres, downloads of the
      boxes), warm, median over the runs;
(ii)  ia3_poly_field_dev at `--shape`, first-order constants on every axis, float64 and float32: kernel time, the store
      rate that is (output bytes / kernel time), and the wall time of the call with its allocation;
(iii) the NumPy / SciPy restatement of both on this machine's CPU (tests/harness/chrom_ref.py: 30 of the pairs, scaled to
      the pair count; generate_polynomial_data and np.dot for one axis of the field, as the reference computes it).
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

from imageanalysis3_amd import _lib as L, synth                                       # noqa: E402
from imageanalysis3_amd.correction_tools.chromatic import generate_polynomial_data    # noqa: E402
from imageanalysis3_amd.io_tools.load import DeviceBuffer                             # noqa: E402


def med(v):
    return float(np.median(np.asarray(v, dtype=np.float64)))


def stage_times(fn, runs, warm=3):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=[50, 2048, 2048])
    ap.add_argument("--pairs", type=int, default=300)
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chromatic.json"))
    a = ap.parse_args()
    shape = tuple(a.shape)
    L.check(L.lib().ia3_init(0))
    name = C.create_string_buffer(256)
    L.lib().ia3_device_name(name, 256)
    res = dict(shape=list(shape), pairs=a.pairs, runs=a.runs, gpu=name.value.decode())

    # (i) boxes and regressions: the stacks need not be large, the kernel reads 11^3 voxels per box
    cshape = (30, 512, 512)
    im_a = synth.make_fov(cshape, 400, 11, dtype=np.uint16)[0]
    im_b = np.clip(0.8 * im_a.astype(np.float64) + 50.0, 0, 65535).astype(np.uint16)
    rng = np.random.RandomState(3)
    ca = rng.rand(a.pairs, 3) * (np.array(cshape) - 1.0)
    cb = np.clip(ca + rng.rand(a.pairs, 3) - 0.5, 0, np.array(cshape) - 1.0)
    with L.DeviceStack.upload(im_a) as sa, L.DeviceStack.upload(im_b) as sb:
        boxes = L.crop_pairs(sa, ca, [9, 9, 9], sb, cb, regress=True)
        s_c, w_c = stage_times(lambda: L.crop_pairs(sa, ca, [9, 9, 9], sb, cb, regress=True), a.runs)
    res["crop_pairs"] = dict(kernel_ms=s_c.get("crop_pairs"), call_wall_ms=w_c, box=[9, 9, 9])
    print(json.dumps(res["crop_pairs"]), flush=True)

    # (ii) the dense field
    consts = [np.array([0.1, 1e-3, 2e-4, -3e-4]), np.array([-0.2, 1e-4, 3e-4, 2e-4]), np.array([0.05, -2e-4, 1e-4, 4e-4])]
    center = np.array(shape) / 2
    res["poly_field"] = {}
    for dt in (np.float64, np.float32):
        def field():
            L.lib().ia3_buffer_free(L.poly_field(consts, [1, 1, 1], center, shape, dt))
        s_f, w_f = stage_times(field, a.runs)
        nbytes = 3 * int(np.prod(shape)) * np.dtype(dt).itemsize
        res["poly_field"][np.dtype(dt).name] = dict(kernel_ms=s_f.get("poly_field"), call_wall_ms=w_f, output_bytes=nbytes,
                                                    store_rate_TBps=nbytes / (s_f["poly_field"] * 1e-3) / 1e12)
    buf = DeviceBuffer.adopt(L.poly_field(consts, [1, 1, 1], center, shape, np.float64), (3,) + shape, np.float64)
    t0 = time.perf_counter()
    dev_field = buf.download()
    res["poly_field"]["download_float64_ms"] = (time.perf_counter() - t0) * 1e3
    buf.free()
    print(json.dumps(res["poly_field"]), flush=True)

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")
    write()

    # (iii) the restatement on the CPU
    if not a.no_cpu:
        from harness import chrom_ref
        m = min(30, a.pairs)
        t0 = time.perf_counter()
        same = True
        for i in range(m):
            xa, xb = chrom_ref.crop_by_scipy(im_a, ca[i], 9), chrom_ref.crop_by_scipy(im_b, cb[i], 9)
            same = same and np.array_equal(xa, boxes[0][i]) and np.array_equal(xb, boxes[1][i])
            chrom_ref.regression_f64(xa, xb)
        t_crop = (time.perf_counter() - t0) / m * a.pairs
        t0 = time.perf_counter()
        grid = np.indices(shape).reshape(3, -1) - center[:, np.newaxis]
        ref = np.dot(generate_polynomial_data(grid.transpose(), 1), consts[0]).reshape(shape)
        t_field = time.perf_counter() - t0
        bound = 4 * 2.0 ** -52 * (np.abs(consts[0][0]) + np.abs(consts[0][1:] * center).sum() * 2)
        res["cpu_numpy"] = dict(crop_pairs_s=t_crop, crops_equal_to_device=bool(same), poly_field_one_axis_s=t_field,
                                poly_field_three_axes_s=3 * t_field,
                                field_within_bound_of_device=bool(np.abs(ref - dev_field[0]).max() <= bound))
        print(json.dumps(res["cpu_numpy"]), flush=True)
        write()


if __name__ == "__main__":
    main()
