"""Times the illumination-profile reduction of one channel stack and the percentile threshold of fit_fov_image.

    python scripts/time_illumination.py [--shape 50 2048 2048] [--runs 25] [--no-cpu] [--out profiles/illumination.json]

(i)   percentile pair, clip-sum and sigma = 60 Gaussian on a resident uint16 stack: per-stage HIP-event times
      (ia3_profile_collect), warm, median over the runs; and the whole ia3_illumination_image_profile_dev call (host wall
      time: the three stages, two small read-backs and the download of the float64 profile);
(ii)  the NumPy restatement of the same reduction (tests/harness/illum_ref.py) on this machine's CPU, one run;
(iii) fit_fov_image(resident float32 stack, use_percentile=True) beside the earlier route of the same call: download
      the stack, two np.partition percentiles on the host, seed from the host copy (a second upload), fit.
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
from imageanalysis3_amd.correction_tools import illumination as I                     # noqa: E402
from imageanalysis3_amd.spot_tools import fitting as F                                # noqa: E402


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
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--spots", type=int, default=5000)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "illumination.json"))
    a = ap.parse_args()
    shape = tuple(a.shape)
    L.check(L.lib().ia3_init(0))
    name = C.create_string_buffer(256)
    L.lib().ia3_device_name(name, 256)
    res = dict(shape=list(shape), runs=a.runs, gpu=name.value.decode())

    f32 = synth.make_fov(shape, a.spots, 7)[0]
    x, y = np.meshgrid(np.arange(shape[1]), np.arange(shape[2]), indexing="ij")
    fall = (1.0 - 0.5 * (((x - 0.45 * shape[1]) / shape[1]) ** 2 + ((y - 0.55 * shape[2]) / shape[2]) ** 2)).astype(np.float32)
    u16 = np.clip(f32 * fall[None] * 4, 0, 65535).astype(np.uint16)
    pers, sigma = [5, 90], 60

    # (i) the stages on the resident uint16 stack
    with L.DeviceStack.upload(u16) as st:
        t0 = time.perf_counter()
        with L.DeviceStack.upload(u16):
            L.check(L.lib().ia3_sync())
        res["upload_ms"] = (time.perf_counter() - t0) * 1e3
        lims = st.percentiles(pers)
        s_per, w_per = stage_times(lambda: st.percentiles(pers), a.runs)

        def clip():
            L.clip_sum_z(st, lims).free()
        s_clip, w_clip = stage_times(clip, a.runs)
        with L.clip_sum_z(st, lims) as summed:
            def gauss():
                L.gaussian_filter2d_f64(summed, sigma).free()
            s_g, w_g = stage_times(gauss, a.runs)
        s_all, w_all = stage_times(lambda: I._stack_to_profile(st, True, pers, sigma), a.runs)
        prof = I._stack_to_profile(st, True, pers, sigma)
    res["device"] = dict(percentile_pair_ms=s_per.get("order_stats"), percentile_pair_wall_ms=w_per,
                         clip_sum_z_ms=s_clip.get("clip_sum_z"), gaussian_sigma60_ms=s_g.get("gaussian2d_f64"),
                         together_stage_sum_ms=sum(s_all.get(k, 0.0) for k in ("order_stats", "clip_sum_z", "gaussian2d_f64")),
                         together_stages_ms=s_all, together_call_wall_ms=w_all, cap_limits=[float(v) for v in lims])
    print(json.dumps(res["device"]), flush=True)

    # (ii) the NumPy restatement on the CPU
    if not a.no_cpu:
        from harness import illum_ref
        t0 = time.perf_counter()
        lo_hi = illum_ref.cap_limits(u16, pers)
        t1 = time.perf_counter()
        summed = illum_ref.clip_sum_z(u16, lo_hi)
        t2 = time.perf_counter()
        ref = illum_ref.gaussian_f64(summed, sigma)
        t3 = time.perf_counter()
        res["cpu_numpy"] = dict(percentile_pair_s=t1 - t0, clip_sum_z_s=t2 - t1, gaussian_sigma60_s=t3 - t2, together_s=t3 - t0,
                                equal_to_device=bool(np.array_equal(ref, prof)))
        print(json.dumps(res["cpu_numpy"]), flush=True)

    # (iii) the percentile threshold in fit_fov_image on a resident float32 stack
    kw = dict(use_percentile=True, th_seed_per=99.5, max_num_seeds=None, verbose=False)
    with L.DeviceStack.upload(f32) as st:
        new, old, parts = [], [], []
        F.fit_fov_image(st, "647", **kw)
        for _ in range(max(3, a.runs // 5)):
            t0 = time.perf_counter()
            t_new = F.fit_fov_image(st, "647", **kw)
            new.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            host = st.download()
            t1 = time.perf_counter()
            th = F._score_at_percentile(host, 99.5) - F._score_at_percentile(host, (100 - 99.5) / 2)
            t2 = time.perf_counter()
            seeds = F.get_seeds(host, th_seed=th, return_h=False)
            t_old = F.fit_fov_image(st, "647", seeds=seeds, max_num_seeds=None, verbose=False)
            t3 = time.perf_counter()
            old.append((t3 - t0) * 1e3)
            parts.append([(t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3])
        t0 = time.perf_counter()
        th_dev = F.stack_percentile_threshold(st, 99.5)
        t_th = (time.perf_counter() - t0) * 1e3
    parts = np.median(np.array(parts), axis=0)
    res["fit_fov_image_percentile"] = dict(resident_device_threshold_ms=med(new), download_and_partition_ms=med(old),
                                           earlier_route_parts_ms=dict(download=float(parts[0]), partition=float(parts[1]),
                                                                       seed_from_host_and_fit=float(parts[2])),
                                           device_threshold_alone_ms=t_th, thresholds_equal=bool(th_dev == th),
                                           spots=[int(len(t_new)), int(len(t_old))])
    print(json.dumps(res["fit_fov_image_percentile"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
