"""Times every public call that runs the radix select (csrc/ia3_select.h) on resident (50, 2048, 2048) stacks.

    python scripts/time_select.py [--shape 50 2048 2048] [--runs 15] [--warmup 3]

One process, warm, a device synchronise around every timed call (host wall time, median over the runs), one JSON line:
ia3_z_shift_correction_dev, ia3_stack_percentiles_dev with two percentiles and ia3_plane_medians_dev on a uint16 and a
float32 stack, ia3_stack_median_dev on the uint16 stack.  `values` carries what the calls returned (the z-shifted stacks
as CRC-32), so that two builds of the library can be compared for equal results as well: IA3_LIB_PATH selects the build.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from imageanalysis3_amd import _lib as L                                              # noqa: E402


def timed(fn, runs, warm):
    for _ in range(warm):
        fn()
    L.check(L.lib().ia3_sync())
    t = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        L.check(L.lib().ia3_sync())
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=[50, 2048, 2048])
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    shape = tuple(a.shape)
    L.check(L.lib().ia3_init(0))
    name = C.create_string_buffer(256)
    L.lib().ia3_device_name(name, 256)

    # camera-like stacks: a narrow background whose level drifts with z, a bright tail
    rng = np.random.default_rng(7)
    u16 = rng.integers(0, 64, shape, dtype=np.uint16)
    u16 += rng.integers(0, 64, shape, dtype=np.uint16)
    u16 += (300 + 4 * np.arange(shape[0], dtype=np.uint16))[:, None, None]
    u16[:, rng.random(shape[1:]) < 0.01] *= 7
    f32 = u16.astype(np.float32) * np.float32(1.01) + np.float32(0.25)
    pers = [0.25, 99.5]

    ms, values = {}, {}
    for tag, im in (("u16", u16), ("f32", f32)):
        with L.DeviceStack.upload(im) as st, L.DeviceStack.empty(shape, np.uint16) as out:
            ms["z_shift_" + tag] = timed(lambda: L.check(L.lib().ia3_z_shift_correction_dev(st._h, out._h)), a.runs, a.warmup)
            values["z_shift_" + tag] = zlib.crc32(out.download().tobytes())
            ms["percentiles_" + tag] = timed(lambda: st.percentiles(pers), a.runs, a.warmup)
            values["percentiles_" + tag] = [float(v) for v in st.percentiles(pers)]
            ms["plane_medians_" + tag] = timed(lambda: L.plane_medians(st), a.runs, a.warmup)
            values["plane_medians_" + tag] = [float(v) for v in L.plane_medians(st)]
            if tag == "u16":
                ms["stack_median_u16"] = timed(lambda: L.stack_median(st), a.runs, a.warmup)
                values["stack_median_u16"] = float(L.stack_median(st))
    print(json.dumps(dict(shape=list(shape), runs=a.runs, gpu=name.value.decode(), lib=os.path.basename(L.LIB_PATH),
                          ms=ms, values=values), sort_keys=True), flush=True)


if __name__ == "__main__":
    main()
