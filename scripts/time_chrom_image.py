"""Times the chromosome image on the device and find_candidate_chromosomes on it.

    python scripts/time_chrom_image.py [--shape 50 2048 2048] [--images 10] [--runs 5] [--cpu-images 2] [--out profiles/chrom_image.json]

(i)   `--images` resident uint16 stacks added into a resident float64 volume as one batch (ia3_chrom_image_add_dev): the
      whole-stack medians (the radix select) and the add kernel separately, HIP events (ia3_profile_collect), warm, median
      over the runs, and the host wall time of the call; beside them the bytes bounds at 6.3 TB/s: (2 K + 16) B per voxel
      for the add, 2 x 2 B per voxel and image for the medians;
(ii)  find_candidate_chromosomes on the resulting ChromImage (ia3_find_candidate_chromosomes_f64_dev), per stage;
(iii) for context, the NumPy statement of the same sum (tests/harness/chromim_ref.py) on `--cpu-images` of the stacks, and
      whether it equals the device's sum of those.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

from imageanalysis3_amd import _lib as L                                              # noqa: E402
from time_chromosome import stage_times, synthetic                                    # noqa: E402

HBM_BYTES_PER_S = 6.3e12   # achievable rate the kernels are judged against


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=[50, 2048, 2048])
    ap.add_argument("--images", type=int, default=10)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--filt-size", type=int, default=4)
    ap.add_argument("--per", type=float, default=99.5)
    ap.add_argument("--min-size", type=int, default=100)
    ap.add_argument("--cpu-images", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chrom_image.json"))
    a = ap.parse_args()
    shape, K = tuple(a.shape), a.images
    nvox = int(np.prod(shape))
    L.check(L.lib().ia3_init(0))
    name = C.create_string_buffer(256)
    L.lib().ia3_device_name(name, 256)
    res = dict(shape=list(shape), images=K, runs=a.runs, gpu=name.value.decode())
    base = synthetic(shape, "u16")
    rng = np.random.RandomState(3)
    drifts = np.round(rng.uniform(-6, 6, size=(K, 3)) * np.array([0.3, 1, 1]), 2).astype(np.float32)
    shifts = np.round(drifts).astype(int)
    flags = np.ones(K, np.int32)
    host = [np.roll(base, k * 37 + 1, axis=2) for k in range(min(K, max(a.cpu_images, 1)))]
    stacks = []
    for k in range(K):
        stacks.append(L.DeviceStack.upload(host[k] if k < len(host) else np.roll(base, k * 37 + 1, axis=2)))
    try:
        with L.ChromImage.empty(shape) as chrom:
            stages, wall = stage_times(lambda: chrom.add(stacks, flags, shifts), a.runs)
            bound_add = (2 * K + 16) * nvox / HBM_BYTES_PER_S * 1e3
            bound_med = K * 4 * nvox / HBM_BYTES_PER_S * 1e3
            res["add"] = dict(call_wall_ms=wall, medians_ms=stages.get("morph_select"), add_ms=stages.get("chrom_add"),
                              add_bound_ms=bound_add, medians_bound_ms=bound_med,
                              add_fraction_of_bound=bound_add / stages["chrom_add"] if stages.get("chrom_add") else None)
            print(json.dumps(res["add"]), flush=True)
        # a fresh image, the batch added once: the input of (ii)
        with L.ChromImage.empty(shape) as chrom:
            chrom.add(stacks, flags, shifts)
            coords, th, _ = L.find_candidate_chromosomes(chrom, a.filt_size, a.per, 1, a.min_size)
            st, w = stage_times(lambda: L.find_candidate_chromosomes(chrom, a.filt_size, a.per, 1, a.min_size), a.runs)
            res["candidates"] = dict(call_wall_ms=w, stages_ms=st, stage_sum_ms=sum(st.values()), objects=int(len(coords)),
                                     threshold=float(th))
            print(json.dumps(res["candidates"]), flush=True)
        if a.cpu_images > 0:
            from harness import chromim_ref as R
            n = min(a.cpu_images, K)
            t0 = time.perf_counter()
            want = R.chrom_im(host[:n], flags[:n], drifts[:n], shape)
            t1 = time.perf_counter()
            with L.ChromImage.empty(shape) as chrom:
                chrom.add(stacks[:n], flags[:n], shifts[:n])
                equal = bool(chrom.download().tobytes() == want.tobytes())
            res["numpy_statement"] = dict(images=n, seconds=t1 - t0, seconds_per_image=(t1 - t0) / n, equal_to_device=equal)
            print(json.dumps(res["numpy_statement"]), flush=True)
    finally:
        for s in stacks:
            s.free()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
