"""Times the density clouds (csrc/cloud.hip) on a nucleus-sized workload.

    python scripts/time_clouds.py [--homologs 46] [--runs 5] [--out profiles/clouds.json]
    python scripts/time_clouds.py --cpu-reference
    python scripts/time_clouds.py --check-count

The workload: one nucleus of `--homologs` homologs (two per chromosome) of 60 loci each, 10 % of them NaN, at the defaults
of convert_chr2Zxys_2_Cloud: 100**3 voxels per homolog and a box of 76**3 per locus.

Without --cpu-reference (needs the GPU): the call warm, median over the runs: the HIP-event time of the kernel
(ia3_profile_collect), the wall time of the library call with its download, and the wall time of the whole function with
the host rules around it.  Reported: (voxel, source) pairs per second, a pair being one evaluated exp (their number is the
sum over the loci of the voxels of their clamped boxes), and the float64 vector instructions they take as a fraction of the
peak of 256 compute units x 64 lanes x 2.4 GHz.  The first homolog is held against the NumPy restatement
(tests/harness/cloud_cases.py) within the float32 bound of DESIGN.md section 27.

INSTR_PER_PAIR is read off the gfx950 assembly and has to be read again when cloud.hip or the compiler changes:

    cd imageanalysis3_amd/csrc && hipcc --offload-arch=gfx950 -O3 -std=c++17 -I../../include -ffp-contract=off \
        --cuda-device-only -S cloud.hip -o cloud.s

In the function whose name holds `cloud_kILb1E` (the float32-rounded kernel) there are two loops marked "Inner Loop Header:
Depth=2": the first fills the tables, the second is the walk over the kept sources; the compiler unrolls it twice, so one
source is half of its body.  Count the vector instructions with an f64 operand (v_*_f64, the v_cvt_* to and from f64) on the
path of a pair inside the box, from the three ds_read_b64 of the terms to the v_cvt_f32_f64 of the accumulator: 3 v_cmp_neq
with the out-of-box mark, 2 v_add and 1 v_mul for the argument, 1 v_cmp for the zero cut, 18 for exp (v_mul, v_rndne, 13
v_fma / v_fmac, v_cvt_i32_f64, v_ldexp, v_cmp), 4 for the float32-rounded add (v_cvt_f64_f32, v_mul, v_add,
v_cvt_f32_f64): 29.  The v_mov_b64 that reload the polynomial's coefficients (9) are not counted.  --check-count compiles as
above and counts the same instructions in that loop, so a change shows without reading the listing.

With --cpu-reference (no GPU): that restatement, which equals the reference bit for bit, on one core for one homolog.
Both parts write into the same JSON file.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

R = 60
INSTR_PER_PAIR = 29
PEAK_LANE_OPS = 256 * 64 * 2.4e9


def make_cell(homologs, seed=0):
    rs = np.random.RandomState(seed)
    cell = {}
    for c in range((homologs + 1) // 2):
        H = min(2, homologs - 2 * c)
        z = rs.uniform(-2.5, 2.5, (H, 1, 3)) + np.cumsum(rs.normal(0, 0.15, (H, R, 3)), axis=1)
        z[rs.rand(H, R) < 0.1] = np.nan
        cell[str(c + 1)] = z
    return cell


def count_instructions():
    """Compiles cloud.hip to gfx950 assembly as the module docstring says and counts, in the second innermost loop of the
    float32-rounded kernel, the vector instructions with an f64 operand per copy of the unrolled body (a copy reads four
    64-bit LDS values: three terms and h)."""
    import re
    import subprocess
    import tempfile
    csrc = os.path.join(ROOT, "imageanalysis3_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "cloud.s")
        subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                               "-ffp-contract=off", "--cuda-device-only", "-S", os.path.join(csrc, "cloud.hip"), "-o", out],
                              stderr=subprocess.DEVNULL)
        lines = open(out).read().splitlines()
    start = next(i for i, l in enumerate(lines) if re.match(r"_Z\w*cloud_kILb1E\w*:", l))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    body = lines[start:end]
    headers = [re.match(r"\.(LBB\d+_\d+):", body[i - 1]).group(1)[1:] for i, l in enumerate(body) if "Inner Loop Header: Depth=2" in l]
    assert len(headers) == 2, headers
    walk, inside, f64, reads = headers[1], False, 0, 0
    for i, l in enumerate(body):
        if re.match(r"(\.LBB\d+_\d+:|; %bb\.\d+:)", l):
            nxt = body[i + 1] if i + 1 < len(body) else ""
            inside = ("Header=%s " % walk) in l or (l.startswith(".L%s:" % walk) and "Inner Loop Header" in nxt)
        elif inside and re.match(r"\tv_\w*f64", l):
            f64 += 1
        elif inside and l.startswith("\tds_read_b64"):
            reads += 1
    assert reads and reads % 4 == 0, reads
    return f64 / (reads // 4)


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
    from harness import cloud_cases as K
    ap = argparse.ArgumentParser()
    ap.add_argument("--homologs", type=int, default=46)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--cpu-reference", action="store_true")
    ap.add_argument("--check-count", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clouds.json"))
    a = ap.parse_args()
    if a.check_count:
        n = count_instructions()
        print("float64 vector instructions per pair: %g (INSTR_PER_PAIR = %d)" % (n, INSTR_PER_PAIR))
        sys.exit(0 if n == INSTR_PER_PAIR else 1)
    cell = make_cell(a.homologs)
    first = {"1": cell["1"][:1]}
    if a.cpu_reference:
        t0 = time.perf_counter()
        K.np_cloud(first)
        dt = time.perf_counter() - t0
        res = dict(homologs=1, loci=int(np.isfinite(first["1"]).all(2).sum()), seconds_per_homolog=dt)
        print(json.dumps(res))
        merge(a.out, "numpy_one_core", res)
        return
    from imageanalysis3_amd import _lib as L
    from imageanalysis3_amd.structure_tools import chromosome as S
    L.check(L.lib().ia3_init(0))
    plan = S._Plan(cell, 0.1, 5, 0.5, [1, 2], 20, 0.25)
    shape = (plan.size,) * 3
    pairs = 0
    for i in range(len(plan.kept)):
        rows = plan.table[plan.image_start[i]:plan.image_start[i + 1]]
        pairs += int(K.contributing(shape, rows[:, :3], rows[:, 4:7], rows[:, 7]).sum())
    out = S.convert_chr2Zxys_2_Cloud(cell)          # warm
    walls, calls, kernels = [], [], []
    for _ in range(a.runs):
        L.profile_enable(True)
        L.profile_collect()
        t0 = time.perf_counter()
        L.cloud_render(plan.table, plan.image_start, shape, rounding=np.float32)
        calls.append(time.perf_counter() - t0)
        kernels.append(L.profile_collect()["cloud"][1] * 1e-3)
        L.profile_enable(False)
        t0 = time.perf_counter()
        S.convert_chr2Zxys_2_Cloud(cell)
        walls.append(time.perf_counter() - t0)
    kernel, call, wall = (float(np.median(v)) for v in (kernels, calls, walls))
    rows = plan.table[:plan.image_start[1]]
    ref = K.np_add_sources(np.zeros(shape, dtype=np.float32), rows[:, :3], 1, rows[:, 4:7], rows[:, 7], rounding=np.float32)
    n = K.contributing(shape, rows[:, :3], rows[:, 4:7], rows[:, 7])
    err = np.abs(out["1"][0].astype(np.float64) - ref.astype(np.float64))
    assert (err <= n * np.spacing(ref)).all()
    res = dict(homologs=len(plan.kept), loci=int(len(plan.table)), pairs=pairs, kernel_s=kernel, call_with_download_s=call,
               function_wall_s=wall, pairs_per_s=pairs / kernel, instructions_per_pair=INSTR_PER_PAIR,
               fp64_vector_fraction=pairs / kernel * INSTR_PER_PAIR / PEAK_LANE_OPS, voxels_that_differ=int((err > 0).sum()),
               output_bytes=int(4 * len(plan.kept) * plan.size**3))
    print(json.dumps(res))
    merge(a.out, "mi355x", res)


if __name__ == "__main__":
    main()
