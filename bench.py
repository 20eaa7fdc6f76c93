#!/usr/bin/env python
"""bench.py — per-FOV spot calling (DoG seed + 3-D Gaussian LM fit) on MI355X.

Contract (driver): `python bench.py --gpus N --steps K --warmup W`; for N>1 either launched through
torch.distributed.run (one rank per GPU, RCCL) or run plainly, in which case it starts the N ranks itself as child
processes before touching the GPU (launch_ranks) and relays rank 0's line.  `--gpus N` and WORLD_SIZE must agree; a result
line that does not report N ranks is an error.  Prints ONE JSON line.

Workload = BASELINE.json configs[1]: 2048x2048x50 float32 FOVs with ~5k spots (synthetic, repo generator
G((50,2048,2048), 5000, seed)).  Every rank keeps `--pool` different FOVs resident in HBM (H2D EXCLUDED from `value`)
and a step = `fit_fov_image` semantics on `--fovs-per-gpu` of them through the C ABI (`ia3_fit_fov_dev`: get_seeds ->
firstfit -> repeatfit -> NaN/boundary row filters), a different FOV every step, spot tables returned to the host.
FOV indices are dealt to the ranks with `parallel.shard_fovs` (weak scaling); the only collective is the final
all-gather of the counts and of the padded [fovs_per_rank, max_seeds, 11] float32 block of every table made in the
timed region, inside the timed region.

value = fitted spots/s over all ranks; `fovs_per_sec` beside it.  Extra objects on the same line:
  roofline      the kernel with the most GPU time in the timed region, by HIP events on the stream it is launched on
                (DESIGN.md §4): the LM fit (counted flop: voxel evaluations x 254, ia3_fit_fov_stats) or a Gaussian launch
                (SciPy's float64 accumulation, bit-identical results); both are f64-VALU-bound -> bound "f64_valu",
                frac = counted flop/s / 78.6 TFLOP/s; roofline_other = the other profiled launches on the same basis
  step_ms       min / median / max of the timed steps (each step ends with its table on the host)
  filter_seed   the whole get_seeds stage on SURVEY §8(d)'s 4 B/voxel basis
  streaming     N=1 only: a different HOST-resident FOV every step, uploaded inside the timed region while others
                compute (`ia3_fit_fovs`), float32 and uint16, next to the measured PCIe bound
  secondary     N=1 only: uint16 FOVs (production dtype), crowded fields (layout B: 5 000 spots in 200 territories, float32
                and uint16), configs[2] (64 FOVs: bead drift by phase correlation + fit) and the single-GPU workload of
                configs[4] (uint16 4-colour movie -> corrections -> drift -> warp -> fit)
  cpu_baseline  the NumPy/SciPy oracle (restatement of the reference's CPU path, pinned against it) on the WHOLE first FOV,
                one core; beside it one window per core on all of this box's cores (N=1 only)
streaming, secondary and cpu_baseline run only with `--full`: a plain run sets up, warms up, times the steps and prints the
line (the objects above it come from the timed steps' own HIP events and counters).

`--dump-outputs DIR` writes, after the timed steps, the spot tables of the last step (what `ia3_fit_fov_dev` hands its
caller: one (n, 11) float32 table per FOV) as DIR/spots_fov<j>.npy, rank 0's only.  The inputs are generated from fixed
seeds, so two builds run with the same arguments can be compared table for table.
"""
import argparse
import json
import mmap
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")   # before anything initialises HIP (streams of the batch workers)

import numpy as np  # noqa: E402

SHAPE = (50, 2048, 2048)
N_SPOTS = 5000
TH_SEED = 600.0
MAX_SEEDS = 8192               # rows per FOV of the gathered block (the reference's max_seeds dimension)
HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8 TB/s spec
F64_VALU_PEAK_TFLOPS = 78.6    # MI355X FP64 vector peak (FMA = 2 flop)
FIT_FLOP_PER_VOXEL_EVAL = 254  # ia3_model.h model_jac + residual + J^T J / J^T r accumulation, exp = 20
DUMP_LIMIT_BYTES = 64 << 20    # --dump-outputs writes at most this much


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shape", type=int, nargs=3, default=list(SHAPE))
    ap.add_argument("--spots", type=int, default=N_SPOTS)
    ap.add_argument("--pool", type=int, default=4, help="different FOVs kept resident per rank")
    ap.add_argument("--fovs-per-gpu", type=int, default=1, help="FOVs per rank per step")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-secondary", action="store_true", help="skip the streaming / uint16 / configs[2] / configs[4] legs")
    ap.add_argument("--cpu-crop", type=int, default=0, help="x/y edge of the CPU baseline's window; 0 = the whole FOV (about a minute on one core)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also the streaming and secondary legs and the CPU baseline (N=1 only)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the spot tables of the last timed step as DIR/spots_fov<j>.npy (float32)")
    return ap.parse_args()


def dump_outputs(dirname, tables):
    """The last timed step's spot tables, one (n, 11) float32 file per FOV in step order.  Should they come to more than
    DUMP_LIMIT_BYTES (a step of very many FOVs), the first ones in step order are written and the rest left out."""
    os.makedirs(dirname, exist_ok=True)
    used = 0
    for j, t in enumerate(tables):
        arr = np.ascontiguousarray(t, dtype=np.float32)
        used += arr.nbytes + 128   # + the .npy header
        if used > DUMP_LIMIT_BYTES:
            break
        np.save(os.path.join(dirname, "spots_fov%d.npy" % j), arr)


# ---------------------------------------------------------------------------------------------------------------------
# host-side synthesis: every stack is generated by a forked worker into an anonymous shared mapping (before this
# process touches the GPU)
# ---------------------------------------------------------------------------------------------------------------------
def _shared(shape, dtype):
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    return np.frombuffer(mmap.mmap(-1, n), dtype=dtype).reshape(shape)


def _gen_worker(kind, args, outs):
    from imageanalysis3_amd import synth
    if kind == "fov":
        shape, n, seed, dtype = args
        outs[0][...] = synth.make_fov(shape, n, seed, dtype=dtype)[0]
    elif kind == "fov_clustered":
        shape, n, seed, dtype = args
        outs[0][...] = synth.make_fov(shape, n, seed, layout="clustered", dtype=dtype)[0]
    elif kind == "beads":
        shape, n, seed, drift, dtype = args
        ref, src, c, h = synth.make_bead_pair(shape, n, seed, drift, dtype=dtype)
        outs[0][...] = ref
        outs[1][...] = src


def generate(jobs, max_procs):
    """jobs: {key: (kind, args, [(shape, dtype), ...])} -> {key: [arrays]}; at most max_procs workers at a time."""
    import multiprocessing as mp
    ctx = mp.get_context("fork")
    out = {k: [_shared(s, d) for s, d in spec[2]] for k, spec in jobs.items()}
    if len(jobs) == 1:   # nothing to overlap: no fork (e.g. under rocprofv3 --pmc, which opens the GPU before main())
        (k, (kind, args, _)), = jobs.items()
        _gen_worker(kind, args, out[k])
        return out
    pending = list(jobs.items())
    running = []
    while pending or running:
        while pending and len(running) < max_procs:
            k, (kind, args, _) = pending.pop(0)
            p = ctx.Process(target=_gen_worker, args=(kind, args, out[k]))
            p.start()
            running.append((k, p))
        k, p = running.pop(0)
        p.join()
        if p.exitcode != 0:
            raise RuntimeError("generator worker for %s failed (exit %s)" % (k, p.exitcode))
    return out


def algorithmic_bytes(kernel, shape, esize=4):
    """ALGORITHMIC HBM bytes of one launch: every dense Gaussian pass reads and writes the stack once
    (8 B/voxel for f32), and so does the fused three-axis short filter; the block-minimum pass and the candidate
    detector read one stack."""
    vox = float(shape[0]) * shape[1] * shape[2]
    if kernel.startswith("gauss_axis0_pair"):
        return 3 * esize * vox                # one stack in, two out
    if kernel.startswith("gauss_axis") or kernel.startswith("gauss_fused3") or kernel.startswith("gauss_xy"):
        return 2 * esize * vox
    if kernel in ("seed_detect", "seed_blockmin"):
        return esize * vox
    return None


def measured_traffic(kernel, shape):
    """HBM bytes per launch of `kernel` from the committed PMC passes (profiles/traffic.json: separate rocprofv3
    --pmc FETCH_SIZE / WRITE_SIZE runs of this same command, gfx950 read correction applied), or None when there is
    no measurement for this kernel and stack shape.  Counters cannot be collected from inside the timed run."""
    try:
        with open(os.path.join(ROOT, "profiles", "traffic.json")) as f:
            t = json.load(f)
        if list(t.get("_shape", [])) != list(shape) or kernel not in t:
            return None
        return int(t[kernel]["read"] + t[kernel]["write"])
    except Exception:
        return None


def launch_ranks(a):
    """`python bench.py --gpus N` without a launcher: start the N ranks as fresh child processes (torch.distributed.run,
    one per GPU) BEFORE this process has made any GPU call, relay rank 0's JSON line, and fail unless that line reports
    N ranks.  (The per-image fan-out this replaces: classes/field_of_view.py:1129-1142.)  Never re-executes a process
    that has touched the GPU: the parent only waits."""
    import socket
    import subprocess
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env["IA3_BENCH_LAUNCHED"] = "1"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=%d" % a.gpus,
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, env=env, text=True)
    line = None
    for ln in proc.stdout:
        t = ln.strip()
        if t.startswith("{") and '"metric"' in t:
            line = t
        else:
            sys.stderr.write(ln)
    rc = proc.wait()
    if rc != 0:
        raise SystemExit("bench.py --gpus %d: a rank failed (launcher exit code %d)" % (a.gpus, rc))
    if line is None:
        raise SystemExit("bench.py --gpus %d: rank 0 printed no result line" % a.gpus)
    got = json.loads(line)
    if got.get("n_gpus") != a.gpus or len(got.get("ms_per_step_by_rank", [])) != a.gpus:
        raise SystemExit("bench.py --gpus %d: the result line reports n_gpus=%r" % (a.gpus, got.get("n_gpus")))
    print(line)


def main():
    a = parse()
    if a.gpus < 1:
        raise SystemExit("bench.py: --gpus must be >= 1")
    if a.steps < 1 or a.warmup < 0:
        raise SystemExit("bench.py: --steps must be >= 1 and --warmup >= 0")
    if "WORLD_SIZE" not in os.environ and a.gpus > 1:
        return launch_ranks(a)
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != a.gpus:
        raise SystemExit("bench.py: --gpus %d but the launcher started WORLD_SIZE=%d ranks" % (a.gpus, world))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    shape = tuple(a.shape)
    full = shape == SHAPE
    extra = world == 1 and a.full and not a.no_secondary
    with_cpu = world == 1 and a.full and not a.no_cpu_baseline
    ncore = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    # ---- host-side work first (forks workers: must precede the first GPU call of this process) ---------------------
    t0 = time.time()
    jobs = {}
    for k in range(a.pool):
        jobs["f32_%d" % k] = ("fov", (shape, a.spots, 3 + rank * a.pool + k, np.float32), [(shape, np.float32)])
    if extra:
        for k in range(3):   # signal channels of the configs[4] movie; the first doubles as the uint16 FOV
            jobs["u16_%d" % k] = ("fov", (shape, a.spots, 40 + k, np.uint16), [(shape, np.uint16)])
        for dt_ in (np.float32, np.uint16):   # layout B: 5 000 spots in 200 territories
            jobs["clu_%s" % np.dtype(dt_).name] = ("fov_clustered", (shape, a.spots, 50, dt_), [(shape, dt_)])
        jobs["beads"] = ("beads", (shape, 300 if full else max(8, shape[1] * shape[2] // 14000), 43, (0.6, -3.4, 5.2), np.uint16), [(shape, np.uint16), (shape, np.uint16)])
    arrs = generate(jobs, max(1, min(ncore, 8) // max(1, world if world <= 8 else 8)))
    fovs = [arrs["f32_%d" % k][0] for k in range(a.pool)]
    gen_s = time.time() - t0
    cpu_base = None
    if with_cpu:
        cpu_base = cpu_baseline(fovs[0], a.cpu_crop)
    forked = None
    if extra:   # children that open the GPU themselves: before this process does
        try:
            forked = forked_pool_leg([arrs["u16_%d" % k][0] for k in range(3)])
        except Exception as e:
            forked = {"error": repr(e)}
    import torch
    import torch.distributed as dist
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device (no CPU fallback)")
    if world > 1 and not os.environ.get("IA3_BENCH_DEVICE") and torch.cuda.device_count() < world:
        raise SystemExit("bench.py --gpus %d: only %d HIP device(s) visible" % (world, torch.cuda.device_count()))
    # rehearsal hooks (one-GPU box): IA3_BENCH_DEVICE pins every rank to one device, IA3_BENCH_BACKEND=gloo swaps
    # the collective backend; the driver's multi-GPU runs set neither
    if os.environ.get("IA3_BENCH_DEVICE"):
        local_rank = int(os.environ["IA3_BENCH_DEVICE"])
    backend = os.environ.get("IA3_BENCH_BACKEND", "nccl")
    torch.cuda.set_device(local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
    from imageanalysis3_amd import _lib as L
    from imageanalysis3_amd.parallel import gather_spot_tables, shard_fovs
    import ctypes as C
    lib = L.lib()
    L.check(lib.ia3_init(local_rank))
    stacks = [L.DeviceStack.upload(im) for im in fovs]
    sp, keep = L.make_seed_params(TH_SEED, max_num_seeds=None)
    fp = L.make_fit_params()
    cap = max(2 * a.spots, MAX_SEEDS)
    F = max(1, a.fovs_per_gpu)
    # FOV indices of the whole job (steps x ranks x F), dealt to the ranks; index -> one of this rank's resident FOVs
    mine = shard_fovs((a.warmup + a.steps) * world * F, rank, world)
    stats = [0, 0, 0]

    row_bufs = [np.empty((cap, 11), dtype=np.float32) for _ in range(a.warmup + a.steps)] if F == 1 else []
    for b in row_bufs:
        b.fill(0)   # touch the pages now: the first write into a fresh buffer would fault them in inside the timed region

    def step(i):
        """FOVs mine[i*F : (i+1)*F]; returns the list of their (n,11) tables and the last (seeds, sweeps)."""
        ids = mine[i * F:(i + 1) * F]
        if F == 1:
            rows = row_bufs[i]   # every step keeps its table (they are all gathered at the end)
            n_rows, n_seeds, n_iter = C.c_int(0), C.c_int(0), C.c_int(0)
            L.check(lib.ia3_fit_fov_dev(stacks[int(ids[0]) % a.pool]._h, C.byref(sp), C.byref(fp), L.ptr(rows), cap,
                                        C.byref(n_rows), C.byref(n_seeds), C.byref(n_iter)))
            st = [C.c_int64(0), C.c_int64(0), C.c_int64(0)]
            lib.ia3_fit_fov_stats(C.byref(st[0]), C.byref(st[1]), C.byref(st[2]))
            for k in range(3):
                stats[k] += st[k].value
            return [rows[:n_rows.value]], (n_seeds.value, n_iter.value)
        tabs, info = L.fit_fovs([stacks[int(j) % a.pool] for j in ids], sp, fp, in_flight=min(F, 4), capacity=cap)
        for d in info:
            stats[0] += d["fits"]; stats[1] += d["nfev"]; stats[2] += d["voxel_evals"]
        return tabs, (info[-1]["n_seeds"], info[-1]["n_iter"])

    def barrier():
        L.check(lib.ia3_sync())
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()

    warm = None
    for i in range(a.warmup):
        warm = step(i)
    if world > 1 and warm is not None:   # untimed: the first collective builds the communicator's rings and staging buffers
        gather_spot_tables(warm[0], MAX_SEEDS, world)
    stats[:] = [0, 0, 0]
    L.profile_enable(True)
    L.profile_collect()
    barrier()
    t0 = time.perf_counter()
    tables = []
    last = (0, 0)
    step_s = []
    for i in range(a.warmup, a.warmup + a.steps):
        ts = time.perf_counter()
        last_tables, last = step(i)   # returns with the step's table on the host: no further synchronisation needed to time it
        step_s.append(time.perf_counter() - ts)
        tables.extend(last_tables)
    # final spot-table all-gather: counts + the padded [fovs_per_rank, max_seeds, 11] f32 block of EVERY table of the
    # timed region (the reference's on-disk layout, field_of_view.py:1361-1382) — the path's only exchange
    table = gather_spot_tables(tables, MAX_SEEDS, world)
    barrier()
    dt = time.perf_counter() - t0
    prof = L.profile_collect()
    L.profile_enable(False)
    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, last_tables)
    total_rows = sum(len(t) for t in tables)
    if world > 1:
        t = torch.tensor([dt, float(total_rows)], dtype=torch.float64,
                         device="cuda" if dist.get_backend() == "nccl" else "cpu")
        tmax = t.clone()
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        tsum = t.clone()
        dist.all_reduce(tsum, op=dist.ReduceOp.SUM)
        dt_max, rows_all = float(tmax[0]), float(tsum[1])
        per_rank = torch.zeros(world, dtype=torch.float64, device=t.device)
        dist.all_gather_into_tensor(per_rank, t[:1].clone())
        rank_ms = [round(float(x) / a.steps * 1e3, 3) for x in per_rank.cpu()]
    else:
        dt_max, rows_all = dt, float(total_rows)
        rank_ms = [round(dt / a.steps * 1e3, 3)]

    out = None
    if rank == 0:
        n_fov = a.steps * F                      # FOVs per rank in the timed region
        ms_per_step = dt_max / a.steps * 1e3
        vox = float(shape[0]) * shape[1] * shape[2]
        stage_ms = {k: v[1] / n_fov for k, v in prof.items()}
        # ---- roofline of the dominant stack-streaming kernel ----------------------------------------------------------
        # the front filter (gauss_fused3_*) and the first pass of the background filter (gauss_axis0_*) run side by side
        # on two streams: each one's event time is its own launch duration WITH the other one on the chip
        if any(k.startswith("gauss_xy") for k in prof):     # DoG pair: the plane-wise passes run next to the block minima
            overlapped = sorted(k for k in prof if k.startswith("gauss_xy") or k == "seed_blockmin")
        else:
            overlapped = sorted(k for k in prof if k.startswith("gauss_fused3") or k.startswith("gauss_axis0")) \
                if any(k.startswith("gauss_fused3") for k in prof) else []
        def gauss_roof(name, n_l, ms_tot):
            """f64-VALU roofline entry of one Gaussian launch: counted flop = NI_Correlate1D's sequence per output
            (w0*x + R x (add, multiply, add)) on every axis the launch runs; instr = the f64 instructions issued."""
            pair = name.startswith("gauss_axis0_pair")     # both axis-0 passes of the DoG pair: radius 30 folded + radius 3
            R = 30 if pair else int(name.split("_R")[1])
            avg_s = ms_tot / n_l * 1e-3
            axes = 3 if name.startswith("gauss_fused3") else (2 if name.startswith("gauss_xy") else 1)
            flop = axes * (1 + 3 * R) * vox + ((1 + 3 * 3) * vox if pair else 0)
            if axes == 1 and R >= 16 and name.startswith("gauss_axis0") and shape[0] in (25, 30, 33, 35, 40, 45, 50, 60):   # Makefile FOLD_DEPTHS
                # column-in-registers form: border folded into the weights, one FMA per plane in reach (gauss.hip)
                per_out = sum(min(shape[0] - 1, z + R) - max(0, z - R) + 1 for z in range(shape[0])) / float(shape[0])
                form = "folded column"
                if pair:
                    per_out += 3 * 3 + 1
                    form = "folded column (radius 30) + radius-3 pass on the same registers"
            elif R >= 16:
                per_out, form = 2 * R + 1, "sliding window, certified fused multiply-add"
            else:
                per_out, form = axes * (3 * R + 1), "unfused multiply and add"
            instr = per_out * vox
            ach = flop / avg_s / 1e12
            gbs = algorithmic_bytes(name, shape) / avg_s / 1e9
            return {"bound": "f64_valu", "kernel": name, "form": form, "achieved": round(ach, 2), "peak": F64_VALU_PEAK_TFLOPS,
                    "unit": "TFLOP/s", "frac": round(ach / F64_VALU_PEAK_TFLOPS, 4),
                    "f64_instr_per_voxel": round(per_out, 1),
                    "issue_frac": round(instr / avg_s / (F64_VALU_PEAK_TFLOPS / 2 * 1e12), 4),
                    "hbm_GBps": round(gbs, 1), "hbm_frac": round(gbs / HBM_PEAK_GBS, 4),
                    "traffic": measured_traffic(name, shape),
                    "algorithmic_bytes": int(algorithmic_bytes(name, shape)), "avg_launch_ms": round(ms_tot / n_l, 4), "launches": n_l,
                    "concurrent_with": [k for k in overlapped if k != name] if name in overlapped else []}
        # longest launch first; a launch that shares the chip with another stream's kernel (its event time is inflated by
        # the overlap) ranks behind the ones that run alone
        dense = sorted(((k, v) for k, v in prof.items() if k.startswith("gauss_")),
                       key=lambda kv: (kv[0] in overlapped and not all(k in overlapped for k in prof if k.startswith("gauss_")),
                                       -kv[1][1] / kv[1][0]))
        roof, roof_other = None, []
        if dense:
            roof = gauss_roof(dense[0][0], *dense[0][1])
            roof["note"] = ("the stack-streaming kernel with the longest launch. scipy.ndimage accumulates in float64 and results "
                            "are kept bit-identical, so the Gaussian passes are bound by f64 vector issue: frac = counted flop/s "
                            "(NI_Correlate1D's sequence) / f64 vector peak, issue_frac = f64 instructions issued / peak issue rate. "
                            "hbm_frac = algorithmic bytes / launch time / 8 TB/s: on float32 stacks the column kernel is close to "
                            "that roof as well (a device copy reaches 5.1 TB/s on the box); the uint16 launch moves half the bytes "
                            "in 0.9 of the time, so issue is the binding limit. traffic = PMC bytes (profiles/traffic.json) to be "
                            "read against algorithmic_bytes; concurrent_with = kernels sharing the chip on a second stream")
            roof_other = [gauss_roof(k, *v) for k, v in dense[1:]]
        # ---- LM fit: counted flops -------------------------------------------------------------------------------------
        fit_ms = sum(v[1] for k, v in prof.items() if k.startswith("fit_"))
        fit_launches = sum(v[0] for k, v in prof.items() if k.startswith("fit_"))
        fit = None
        if fit_ms > 0 and stats[2] > 0:
            fl = stats[2] * float(FIT_FLOP_PER_VOXEL_EVAL)
            ach = fl / (fit_ms * 1e-3) / 1e12
            wait_c, wave_c = C.c_int64(0), C.c_int64(0)
            lib.ia3_fit_fov_wait_share(C.byref(wait_c), C.byref(wave_c))
            fit = {"bound": "f64_valu", "kernel": "fit_stages_k", "achieved": round(ach, 2), "peak": F64_VALU_PEAK_TFLOPS,
                   "unit": "TFLOP/s", "frac": round(ach / F64_VALU_PEAK_TFLOPS, 4),
                   "traffic": measured_traffic("fit_first", shape),
                   "algorithmic_bytes": int(stats[0] / n_fov * 2048 + stats[0] / n_fov / 2 * (104 + 44)),
                   "avg_launch_ms": round(fit_ms / max(1, fit_launches), 4), "launches": fit_launches,
                   "ms_per_fov": round(fit_ms / n_fov, 4),
                   "fits_per_fov": round(stats[0] / n_fov, 1), "evaluations_per_fit": round(stats[1] / max(1, stats[0]), 2),
                   "voxels_per_evaluation": round(stats[2] / max(1, stats[1]), 1),
                   "flop_per_voxel_evaluation": FIT_FLOP_PER_VOXEL_EVAL, "gflop_per_fov": round(fl / n_fov / 1e9, 3),
                   "waves_per_simd": 2, "registers_per_wave": 256,
                   "simd_us_per_evaluation": round(fit_ms * 1e3 * 1024 / max(1, stats[1]), 2),
                   "dependency_wait_share_last_fov": round(wait_c.value / max(1, wave_c.value), 4),
                   "note": "algorithmic flops only (residual, float32-rounded Jacobian row, J^T J and J^T r per voxel, 254 per voxel "
                           "and evaluation); the 10x10 trust-region algebra every wave runs is not counted. One wave per fit, two "
                           "persistent waves per SIMD (256 registers each), work handed out by ticket counters; not HBM-bound "
                           "(2 KB gathered per fit: algorithmic_bytes) and not MFMA-shaped (f64 MFMA shares the vector unit's "
                           "datapath on gfx950); simd_us_per_evaluation = kernel time x 1024 SIMDs / evaluations"}
        # the roofline object of the contract = the kernel with the most GPU time in the timed region
        cands = []
        if fit is not None:
            cands.append((fit_ms, fit))
        if roof is not None:
            cands.append((dense[0][1][1], roof))
        cands += [(v[1], r) for (k, v), r in zip(dense[1:], roof_other)]
        cands.sort(key=lambda kv: -kv[0])
        roof = cands[0][1] if cands else None
        roof_other = [r for _, r in cands[1:]]
        seed_keys = [k for k in stage_ms if k.startswith("gauss") or k.startswith("seed_")]
        filt_seed_ms = sum(stage_ms[k] for k in seed_keys if k not in overlapped)
        if overlapped:
            filt_seed_ms += max(stage_ms[k] for k in overlapped)   # the two overlapped launches share their wall time
        vox_bytes = 4.0 * vox
        out = {
            "metric": "fitted spots/sec (+ FOVs/sec), 2048x2048x50 float32 stack, ~5k spots/FOV",
            "value": round(rows_all / dt_max, 1), "unit": "spots/s",
            "fovs_per_sec": round(world * n_fov / dt_max, 3),
            "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": round(ms_per_step, 3),
            "step_ms": {"min": round(min(step_s) * 1e3, 3), "median": round(float(np.median(step_s)) * 1e3, 3),
                        "max": round(max(step_s) * 1e3, 3), "note": "rank 0, host clock around each step (its table is on the host when it returns)"},
            "ms_per_step_by_rank": rank_ms,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f64",
            "data": "synthetic",
            "config": {"workload": "configs[1]: %dx%dx%d float32 FOVs, %d injected spots each, DoG seed + LM fit"
                                   % (shape[1], shape[2], shape[0], a.spots),
                       "input": "resident in HBM, H2D excluded (see streaming for the H2D-inclusive rate)",
                       "fovs_per_gpu_per_step": F, "distinct_fovs_per_gpu": a.pool, "th_seed": TH_SEED,
                       "parallelism": "fov-shard x%d" % world,
                       "spots_last_fov": int(len(tables[-1])), "seeds_last_fov": last[0], "repeat_sweeps": last[1],
                       "gathered_block": [int(world * n_fov), MAX_SEEDS, 11],
                       "gathered_table_rows": int(table.shape[0]) if table is not None else None},
            "roofline": roof,
            "roofline_other": roof_other,
            "stage_ms_per_fov": {k: round(v, 4) for k, v in sorted(stage_ms.items())},
            "stages_overlapped": overlapped,
            "filter_seed": {"ms_per_fov": round(filt_seed_ms, 4),
                            "algorithmic_GBps": round(vox_bytes / (filt_seed_ms * 1e-3) / 1e9, 1) if filt_seed_ms else None,
                            "frac_of_hbm_peak": round(vox_bytes / (filt_seed_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) if filt_seed_ms else None,
                            "note": "background filter evaluated lazily: axis-0 pass on the whole stack, axes 1 and 2 only around "
                                    "candidate maxima (seed.hip); seeds identical to the dense filter"},
            "host_gen_s": round(gen_s, 1),
        }
        if extra:
            try:
                out["streaming"] = streaming_legs(L, fovs, arrs["u16_0"][0], sp, fp)
            except Exception as e:   # the contract line must still come out
                out["streaming"] = {"error": repr(e)}
            try:
                out["secondary"] = secondary_legs(L, stacks, arrs, sp, fp, shape)
            except Exception as e:
                out["secondary"] = {"error": repr(e)}
            if isinstance(out["secondary"], dict) and forked is not None:
                u = out.get("streaming", {}).get("u16", {})
                if "fovs_per_sec" in forked and "fovs_per_sec" in u:
                    forked["batch_entry_fovs_per_sec"] = u["fovs_per_sec"]
                    forked["frac_of_batch_entry"] = round(forked["fovs_per_sec"] / u["fovs_per_sec"], 3)
                out["secondary"]["forked_pool"] = forked
        if a.full and not a.no_cpu_baseline:
            out["cpu_baseline"] = cpu_base   # None for multi-GPU runs (measured at N=1 only)
    for s in stacks:
        s.free()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        print(json.dumps(out))


# ---------------------------------------------------------------------------------------------------------------------
# N=1 extras (after the contract's timed region)
# ---------------------------------------------------------------------------------------------------------------------
def _pcie_GBps(L, im):
    """H2D rate of one ia3_stack_upload of `im` (best of 3): the PCIe bound the streaming rate is compared with."""
    best = None
    for _ in range(3):
        t0 = time.perf_counter()
        st = L.DeviceStack.upload(im)
        dt = time.perf_counter() - t0
        st.free()
        best = dt if best is None or dt < best else best
    return im.nbytes / best / 1e9


def streaming_legs(L, f32_fovs, u16_fov, sp, fp):
    """A different host-resident FOV every step, uploaded inside the timed region: `ia3_fit_fovs` keeps several FOVs in
    flight on library-owned threads and streams, so the upload of one overlaps the filters and fits of the others."""
    res = {}
    u16s = [u16_fov, u16_fov[:, ::-1], u16_fov[:, :, ::-1], u16_fov[::-1]]   # four different uint16 FOVs from one
    u16s = [np.ascontiguousarray(x) for x in u16s]
    for name, ims, depth, n in (("f32", f32_fovs, 3, 12), ("u16", u16s, 8, 96)):   # groups of `depth` images (one fitter per group)
        bw = _pcie_GBps(L, ims[0])
        batch = [ims[k % len(ims)] for k in range(n)]
        L.fit_fovs(batch[:depth], sp, fp, in_flight=depth)   # warm: worker threads, their streams and scratch
        L.check(L.lib().ia3_sync())
        t0 = time.perf_counter()
        tabs, info = L.fit_fovs(batch, sp, fp, in_flight=depth)
        dt = time.perf_counter() - t0
        bound = bw * 1e9 / ims[0].nbytes
        res[name] = {"fovs": n, "in_flight": depth, "ms_per_fov": round(dt / n * 1e3, 3), "fovs_per_sec": round(n / dt, 2),
                     "spots_per_sec": round(sum(len(t) for t in tabs) / dt, 1),
                     "h2d_GBps_inside": round(ims[0].nbytes * n / dt / 1e9, 2), "pcie_GBps_measured": round(bw, 2),
                     "pcie_bound_fovs_per_sec": round(bound, 2), "frac_of_pcie_bound": round(n / dt / bound, 3),
                     "MB_per_fov": round(ims[0].nbytes / 1e6, 1)}
    res["note"] = ("host ndarray -> pageable hipMemcpy (56 GB/s measured, same as pinned) on a worker thread while other "
                   "workers compute; value/fovs_per_sec of the headline exclude this transfer")
    return res


def secondary_legs(L, f32_stacks, arrs, sp, fp, shape):
    import ctypes as C
    lib = L.lib()
    res = {}
    # ---- the headline FOVs through the batch entry: one caller thread, groups of images share a fitter, the seed stage of
    # the next group runs beside the fit of this one (the headline above makes one synchronous call per FOV) --------------
    L.fit_fovs([f32_stacks[k % len(f32_stacks)] for k in range(64)], sp, fp, in_flight=32)
    n = 128
    t0 = time.perf_counter()
    tabs, info = L.fit_fovs([f32_stacks[k % len(f32_stacks)] for k in range(n)], sp, fp, in_flight=32)
    dt = time.perf_counter() - t0
    res["f32_fov_batched"] = {"workload": "configs[1] FOVs (float32, resident) through ia3_fit_fovs: %d images, groups of 32" % n,
                              "batched_in_flight": 32, "batched_fovs": n, "batched_ms_per_fov": round(dt / n * 1e3, 3),
                              "batched_spots_per_sec": round(sum(len(t) for t in tabs) / dt, 1),
                              "note": "same tables as one call per image (tests); host gaps and the seed stage of the next group "
                                      "overlap the fit"}
    # ---- production dtype: uint16 FOV, resident ---------------------------------------------------------------------
    u16 = arrs["u16_0"][0]
    with L.DeviceStack.upload(u16) as st:
        rows = np.empty((MAX_SEEDS * 2, 11), np.float32)
        nr, ns, ni = C.c_int(0), C.c_int(0), C.c_int(0)
        ts = []
        for _ in range(3):
            L.check(lib.ia3_sync()); t0 = time.perf_counter()
            L.check(lib.ia3_fit_fov_dev(st._h, C.byref(sp), C.byref(fp), L.ptr(rows), len(rows), C.byref(nr), C.byref(ns), C.byref(ni)))
            ts.append(time.perf_counter() - t0)
        L.fit_fovs([st] * 32, sp, fp, in_flight=32)
        n = 128   # four groups of 32: the two fitter threads of the batch entry overlap one group's tail with the next group
        t0 = time.perf_counter()
        tabs, info = L.fit_fovs([st] * n, sp, fp, in_flight=32)
        dt = time.perf_counter() - t0
        res["u16_fov"] = {"workload": "configs[1] FOV as uint16 (production dtype), resident",
                          "one_stream_ms_per_fov": round(min(ts) * 1e3, 2), "seeds": ns.value, "rows": nr.value, "sweeps": ni.value,
                          "batched_in_flight": 32, "batched_fovs": n, "batched_ms_per_fov": round(dt / n * 1e3, 3),
                          "batched_spots_per_sec": round(sum(len(t) for t in tabs) / dt, 1),
                          "note": "plateau-duplicate seeds refit noise to maxfev=1000 in every sweep (same in the reference): a "
                                  "lone FOV waits for those fits; ia3_fit_fovs fits a group of images with one fitter, "
                                  "so those waves work beside the other images' fits"}
    # ---- crowded fields (SURVEY.md §8d layout B): several dependent refit sweeps, exact Voronoi ties, stragglers -------
    for key in ("clu_float32", "clu_uint16"):
        if key not in arrs:
            continue
        with L.DeviceStack.upload(arrs[key][0]) as st:
            rows = np.empty((MAX_SEEDS * 2, 11), np.float32)
            nr, ns, ni = C.c_int(0), C.c_int(0), C.c_int(0)
            ts = []
            for _ in range(2):
                L.check(lib.ia3_sync())
                L.profile_enable(True); L.profile_collect()
                t0 = time.perf_counter()
                L.check(lib.ia3_fit_fov_dev(st._h, C.byref(sp), C.byref(fp), L.ptr(rows), len(rows), C.byref(nr), C.byref(ns), C.byref(ni)))
                ts.append(time.perf_counter() - t0)
                prof = L.profile_collect(); L.profile_enable(False)
            st3 = [C.c_int64(0), C.c_int64(0), C.c_int64(0)]
            lib.ia3_fit_fov_stats(C.byref(st3[0]), C.byref(st3[1]), C.byref(st3[2]))
            wc, wv = C.c_int64(0), C.c_int64(0)
            lib.ia3_fit_fov_wait_share(C.byref(wc), C.byref(wv))
            L.fit_fovs([st] * 32, sp, fp, in_flight=32)
            n = 128
            t0 = time.perf_counter()
            tabs, info = L.fit_fovs([st] * n, sp, fp, in_flight=32)
            dt = time.perf_counter() - t0
            fit_ms = sum(v[1] for k, v in prof.items() if k.startswith("fit_"))
            res["clustered_" + key.split("_")[1]] = {
                "workload": "layout B: %d spots in 200 territories, %s, resident" % (N_SPOTS, key.split("_")[1]),
                "one_stream_ms_per_fov": round(min(ts) * 1e3, 2), "seeds": ns.value, "rows": nr.value, "sweeps": ni.value,
                "fit_ms": round(fit_ms, 2), "voronoi_ties_ms": round(sum(v[1] for k, v in prof.items() if k == "voronoi_ties"), 3),
                "fits": st3[0].value, "evaluations": st3[1].value,
                "dependency_wait_share": round(wc.value / max(1, wv.value), 4),
                "batched_in_flight": 32, "batched_fovs": n, "batched_ms_per_fov": round(dt / n * 1e3, 3),
                "batched_spots_per_sec": round(sum(len(t) for t in tabs) / dt, 1),
                "note": "exact Voronoi ties resolved by the reference's cKDTree rule (seed tree built on the host, queries on the "
                        "device); the sweeps are the reference's ordered Gauss-Seidel: a lone FOV waits for its chains of dependent "
                        "refits and for the few fits that run to maxfev, a batch overlaps them"}
    # ---- configs[2]: drift of a bead FOV against the reference bead FOV (phase correlation) + fit of the signal FOV ----
    from imageanalysis3_amd.correction_tools.alignment import align_image, DriftReference
    ref_b, src_b = arrs["beads"]
    with L.DeviceStack.upload(ref_b) as dref_stack, L.DeviceStack.upload(src_b) as dsrc:
        dref = DriftReference(dref_stack)   # the run's reference bead FOV: its crop spectra are made once
        # eight different bead FOVs (the generated one moved by whole pixels: eight different drifts), resident
        shifts = [(k, -2 * k) for k in range(8)]
        dsrcs = [dsrc] + [L.DeviceStack.upload(np.roll(src_b, sh, axis=(1, 2))) for sh in shifts[1:]]
        kw_al = dict(use_autocorr=True, verbose=False, correction_args={'single_im_size': shape})
        align_image(dsrc, dref, **kw_al)
        n = 64   # the batch configs[2] names (the signal FOVs cycle through the resident ones, the bead FOVs through eight)
        L.check(lib.ia3_sync()); t0 = time.perf_counter()
        t_align = 0.0
        n_rows = 0
        drifts, flags = [], []
        for k in range(n):
            ta = time.perf_counter()
            drift, flag = align_image(dsrcs[k % 8], dref, **kw_al)
            t_align += time.perf_counter() - ta
            if k < 8:
                drifts.append([round(float(x), 3) for x in drift]); flags.append(int(flag))
            nr = C.c_int(0)
            L.check(lib.ia3_fit_fov_dev(f32_stacks[k % len(f32_stacks)]._h, C.byref(sp), C.byref(fp), L.ptr(rows), len(rows),
                                        C.byref(nr), None, None))
            n_rows += nr.value
        dt = time.perf_counter() - t0
        for k in range(1, 8):   # a bead FOV moved by (a, b) pixels must come out with the drift moved by (-a, -b), up to the
            #                        beads that enter and leave the (fixed) crop windows at their edges
            want = [drifts[0][0], drifts[0][1] - shifts[k][0], drifts[0][2] - shifts[k][1]]
            if max(abs(a_ - b_) for a_, b_ in zip(drifts[k], want)) > 0.15:
                raise RuntimeError("configs[2] leg: drift of the moved bead FOV %d is %s, expected %s" % (k, drifts[k], want))
        # kernel time of one alignment (HIP events on the calling thread's stream) against its two roofs
        L.profile_enable(True); L.profile_collect()
        for k in range(8):
            align_image(dsrcs[k], dref, **kw_al)
        L.check(lib.ia3_sync())
        prof = L.profile_collect(); L.profile_enable(False)
        cz, cx, cy = shape[0], max(shape) // 4, max(shape) // 4
        cx, cy = min(cx, shape[1]), min(cy, shape[2])
        Ncrop = float(cz * cx * cy)
        n_crops_used = prof.get("xcorr_fft", (0, 0.0))[0] / 8.0
        fft_ms = prof.get("xcorr_fft", (0, 0.0))[1] / 8.0
        dft_ms = prof.get("xcorr_dft", (0, 0.0))[1] / 8.0
        R = 150
        dft_flop = 8.0 * (R * cz * cx * ((cy - 1) // 2) + R * R * cz * cx + R * R * R * cz)   # complex multiply-adds x 8
        fft_bytes = 2 * (3 * 2 * 8 * Ncrop)    # two transforms per crop (the reference crop's spectrum is kept), SURVEY 8(d)'s 3 passes
        res["c3_drift_fit"] = {
            "workload": "configs[2], 64 FOVs one after the other from one host thread; per FOV: align_image (8 crops of 50x512x512, x100 "
                        "upsampled phase correlation, early exit at 3 consistent crops) of a resident uint16 bead FOV (eight different "
                        "ones, cycled) against the run's reference bead FOV (DriftReference: its crop spectra are kept) + seed/fit "
                        "of a float32 FOV",
            "fovs": n, "ms_per_fov": round(dt / n * 1e3, 3), "align_ms": round(t_align / n * 1e3, 3),
            "fit_ms": round((dt - t_align) / n * 1e3, 3), "fovs_per_sec": round(n / dt, 2), "spots_per_sec": round(n_rows / dt, 1),
            "drifts": drifts, "flags": flags, "injected": [-0.6, 3.4, -5.2], "bead_fov_moved_by_px": shifts,
            "roofline": {"crops_per_alignment": n_crops_used, "kernel_ms_per_alignment": round(fft_ms + dft_ms, 3),
                         "fft": {"bound": "hbm", "ms": round(fft_ms, 3), "algorithmic_GB": round(fft_bytes * n_crops_used / 1e9, 3),
                                 "achieved": round(fft_bytes * n_crops_used / 1e9 / (fft_ms * 1e-3), 1) if fft_ms else None, "peak": 8000.0,
                                 "unit": "GB/s", "frac": round(fft_bytes * n_crops_used / 1e9 / (fft_ms * 1e-3) / 8000.0, 4) if fft_ms else None,
                                 "note": "crop -> float64, D2Z of the bead crop, cross-power, Z2D, argmax; 3 x 2 x 8 N bytes per transform "
                                         "(SURVEY 8d), N = 50 x 512 x 512"},
                         "upsampled_dft": {"bound": "mfma_f64", "ms": round(dft_ms, 3), "gflop": round(dft_flop * n_crops_used / 1e9, 2),
                                           "achieved": round(dft_flop * n_crops_used / 1e12 / (dft_ms * 1e-3), 2) if dft_ms else None,
                                           "peak": F64_VALU_PEAK_TFLOPS, "unit": "TFLOP/s",
                                           "frac": round(dft_flop * n_crops_used / 1e12 / (dft_ms * 1e-3) / F64_VALU_PEAK_TFLOPS, 4) if dft_ms else None,
                                           "note": "three complex contractions (150 x N_axis) on v_mfma_f64_16x16x4, the first over half "
                                                   "the columns (Hermitian completion); f64 matrix peak = f64 vector peak on gfx950"}}}
        # the same 64 FOVs from two host threads (each with its own streams): the drift of one FOV overlaps the fit of another
        from concurrent.futures import ThreadPoolExecutor
        def one_fov(k):
            drift_k, flag_k = align_image(dsrcs[k % 8], dref, **kw_al)
            rr = np.empty((MAX_SEEDS * 2, 11), np.float32)
            nk = C.c_int(0)
            L.check(lib.ia3_fit_fov_dev(f32_stacks[k % len(f32_stacks)]._h, C.byref(sp), C.byref(fp), L.ptr(rr), len(rr), C.byref(nk), None, None))
            return nk.value
        with ThreadPoolExecutor(max_workers=2) as pool2:
            list(pool2.map(one_fov, range(4)))
            L.check(lib.ia3_sync()); t0 = time.perf_counter()
            rows2 = sum(pool2.map(one_fov, range(n)))
            dt2 = time.perf_counter() - t0
        res["c3_drift_fit"]["two_host_threads"] = {"fovs": n, "ms_per_fov": round(dt2 / n * 1e3, 3), "fovs_per_sec": round(n / dt2, 2),
                                                   "spots_per_sec": round(rows2 / dt2, 1)}
        for s_ in dsrcs[1:]:
            s_.free()
        dref.free()
    # ---- configs[4], one GPU: uint16 4-colour movie -> corrections -> drift -> warp -> fit ---------------------------
    from imageanalysis3_amd.io_tools.load import correct_fov_image, DeviceBuffer
    Z, X, Y = shape
    chs = ['750', '647', '561', '488']
    raw = np.empty((4 * Z, X, Y), np.uint16)
    for i in range(3):
        raw[i::4] = arrs["u16_%d" % i][0]
    raw[3::4] = src_b
    yy, xx = np.meshgrid(np.linspace(-1, 1, Y), np.linspace(-1, 1, X))
    bump = (0.55 + 0.45 * np.exp(-(xx ** 2 + yy ** 2))).astype(np.float32)
    illum = {c: DeviceBuffer(bump) for c in chs}
    bleed = np.zeros((3, 3, X, Y), np.float32)
    for p in range(3):
        for q in range(3):
            bleed[p, q] = 1.0 if p == q else 0.05
    bleed = DeviceBuffer(bleed)
    zz = np.linspace(-1, 1, Z, dtype=np.float32)[:, None, None]
    field = np.stack([0.2 * zz + 0 * xx[None].astype(np.float32), (0.8 * xx[None] + 0 * zz).astype(np.float32),
                      (0.8 * yy[None] + 0 * zz).astype(np.float32)]).astype(np.float32)
    chrom = {'750': DeviceBuffer(field), '647': None, '561': DeviceBuffer(-field)}
    import contextlib
    import io
    with L.DeviceStack.upload(ref_b) as dref:
        rows_seen = set()
        def movie():
            # the per-movie path (one call per movie, as round 3 measured it): correct_fov_image, then its three channels
            # verbose=True is what makes the reference warp (load.py:434-453); its prints go to the sink opened below
            ims, drift, flag = correct_fov_image(raw, chs[:3], single_im_size=[Z, X, Y], all_channels=chs,
                                                 num_buffer_frames=0, num_empty_frames=0, calculate_drift=True,
                                                 ref_filename=dref, corr_channels=chs[:3], illumination_profile=illum,
                                                 bleed_profile=bleed, chromatic_profile=chrom, warp_image=True,
                                                 return_drift=True, return_device=True, verbose=True)
            try:
                tabs, info = L.fit_fovs(ims, sp, fp, in_flight=3)
            finally:
                for s in ims:
                    s.free()
            rows_seen.add(tuple(len(t) for t in tabs))   # the same movie every time: one row count per channel
            return sum(len(t) for t in tabs), drift
        sink = contextlib.redirect_stdout(io.StringIO())   # ONE redirection around all movies (it is not thread-safe)
        sink.__enter__()
        try:
            per_movie = _c5_runs(L, lib, movie)
        finally:
            sink.__exit__(None, None, None)
        if len(rows_seen) != 1:
            raise RuntimeError("configs[4] leg: the same movie gave different tables: %s" % sorted(rows_seen))
        # ---- the pipelined entry: ONE caller thread, ia3_process_movies over a batch of movies ---------------------------
        # three different movies (the signal channels rotated, the bead channel shifted by whole pixels), cycled
        from imageanalysis3_amd.io_tools.load import MoviePlan
        raws = [raw]
        for k in (1, 2):
            r_ = np.empty_like(raw)
            for i in range(3):
                r_[i::4] = arrs["u16_%d" % ((i + k) % 3)][0]
            r_[3::4] = np.roll(src_b, (k, -2 * k), axis=(1, 2))
            raws.append(r_)
        plan = MoviePlan(chs[:3], ref_image=dref, single_im_size=[Z, X, Y], all_channels=chs, num_buffer_frames=0,
                         num_empty_frames=0, calculate_drift=True, corr_channels=chs[:3], illumination_profile=illum,
                         bleed_profile=bleed, chromatic_profile=chrom, warp_image=True, verbose=True,
                         seed_th={c: TH_SEED for c in chs[:3]}, fitting_args=dict(max_num_seeds=None), frames=4 * Z)
        n_mov = 24
        # warm with a batch of the same length: pool threads, their streams, FFT plans and every scratch block the full
        # pipeline depth needs (a six-movie warm-up left two 1.7 GB blocks to the timed batch: 72 ms of hipMalloc each with
        # all streams stalled, profiles/r04u; `scratch_cache` below reports the calls inside the timed region)
        plan.run([raws[k % 3] for k in range(n_mov)])
        ws0 = (C.c_double * 6)(); ws1 = (C.c_double * 6)()
        L.check(lib.ia3_workspace_stats(ws0))
        L.check(lib.ia3_sync()); t0 = time.perf_counter()
        out = plan.run([raws[k % 3] for k in range(n_mov)])
        dt = time.perf_counter() - t0
        L.check(lib.ia3_workspace_stats(ws1))
        if tuple(len(t) for t in out[0]["tables"]) != sorted(rows_seen)[0]:
            raise RuntimeError("configs[4] leg: the pipelined entry and the per-movie path disagree on movie 0: %s vs %s"
                               % ([len(t) for t in out[0]["tables"]], sorted(rows_seen)[0]))
        for k in range(3, n_mov):
            if [len(t) for t in out[k]["tables"]] != [len(t) for t in out[k % 3]["tables"]] or not np.array_equal(out[k]["drift"], out[k % 3]["drift"]):
                raise RuntimeError("configs[4] leg: the same movie gave different results inside one batch")
        bw = _pcie_GBps(L, raw)
        spots = sum(len(t) for o in out for t in o["tables"])
        c5 = {"workload": per_movie["workload"],
              "entry": "ia3_process_movies through io_tools.load.MoviePlan (what batch_process_images_to_spots calls): one caller "
                       "thread; library threads upload movie k+1 | corrections, drift, warps, get_seeds of movies k, k-1 | one "
                       "group fit over the channels of four movies (fill and drain of the pipeline inside the timed region)",
              "movies": n_mov, "distinct_movies": 3, "s_per_movie": round(dt / n_mov, 4),
              "images_per_sec": round(3 * n_mov / dt, 2), "spots_per_sec": round(spots / dt, 1),
              "drifts": [[round(float(x), 3) for x in out[k]["drift"]] for k in range(3)],
              "MB_per_movie": round(raw.nbytes / 1e6, 1), "pcie_GBps_measured": round(bw, 2),
              "pcie_bound_s_per_movie": round(raw.nbytes / 1e9 / bw, 4),
              "frac_of_pcie_bound": round(raw.nbytes / 1e9 / bw / (dt / n_mov), 3),
              "rows_per_channel": [len(t) for t in out[0]["tables"]],
              "stage_ms_per_movie": {k_: round(float(np.mean([o["ms"][k_] for o in out])), 2) for k_ in ("upload", "correct", "fit")},
              "stage_note": "host wall time a movie spends in each stage (they overlap: upload on one thread, corrections on "
                            "two, fits on one); correct = split + hot pixels + bleedthrough + illumination + drift + 3 warps + "
                            "3 get_seeds; fit = its share of the group fits",
              "scratch_cache": {"idle_GB": round(ws1[0] / 1e9, 1), "in_use_GB": round(ws1[1] / 1e9, 1), "blocks": int(ws1[2]),
                                "hipMalloc_in_timed_region": int(ws1[3] - ws0[3]), "hipFree_in_timed_region": int(ws1[4] - ws0[4]),
                                "ms_in_both": round(ws1[5] - ws0[5], 2)},
              "timeline_ms": [[round(v, 2) for v in o["stamps"]] for o in out],
              "per_movie_calls": {"one_host_thread_s_per_movie": per_movie["s_per_movie"],
                                  "three_host_threads_s_per_movie": per_movie["three_host_threads"]["s_per_movie"],
                                  "note": "the round-3 path: correct_fov_image + fit of the movie's own three channels, one "
                                          "call per movie"}}
        c5["warp"] = _warp_block(L, lib, arrs["u16_0"][0], chrom['750'], (float(field[0].min()), float(field[0].max())))
        res["c5_movie"] = c5
    return res


def _warp_block(L, lib, im, field_buf, fz_range=(0.0, 0.0)):
    """The cubic warp of one channel on its own (resident uint16 stack, drift + dense float32 chromatic field): HIP-event
    time of each of its kernels and where that stands against HBM and the f64 vector unit.  `algorithmic` is what a warp
    has to move (stack in, field in, stack out); `prefilter_moves` is what SciPy's float64 spline prefilter costs on top
    when it is kept exact: the padded float64 coefficient stack written once by the z pass, read and written ONCE by each
    of the two long axes (round 3: the anticausal recursion of a tile starts from a value certified by two bounding
    chains, csrc/warp.hip; the two-sweep form moved it twice) and read once by the gather.  The gather is not a memory
    kernel: SciPy sums 64 products per output, each three multiplications and one addition in float64 in a fixed order
    (256 operations) after ~105 for the three axes' weights; `gather.frac` is that count against the non-fused float64 issue rate."""
    import ctypes as C
    Z, X, Y = im.shape
    drift = np.array([-0.6, 3.4, -5.17])
    with L.DeviceStack.upload(im) as src, L.DeviceStack.empty(im.shape, im.dtype) as dst:
        def run():
            L.check(lib.ia3_warp3d_dev(src._h, L.dptr(drift), field_buf.ptr, field_buf.dtype_code, 3, L.MODE_NEAREST,
                                       C.c_double(0.0), dst._h))
        run(); L.check(lib.ia3_sync())
        ts = []
        for _ in range(5):
            t0 = time.perf_counter(); run(); L.check(lib.ia3_sync()); ts.append(time.perf_counter() - t0)
        L.profile_enable(True)
        n = 5
        for _ in range(n):
            run()
        L.check(lib.ia3_sync())
        prof = L.profile_collect()
        L.profile_enable(False)
    k_ms = {k: round(v[1] / v[0], 4) for k, v in prof.items() if k.startswith("spline_") or k == "warp_cubic"}
    V = Z * X * Y
    # the padded planes the prefilter computes: those a tap of the gather can reach (csrc/warp.hip, zrange_k) — from the
    # drift and the range of the field's z component, as the library derives them
    lo = fz_range[0] - (1e-4 + 1e-6 * abs(fz_range[0]))
    hi = fz_range[1] + (1e-4 + 1e-6 * abs(fz_range[1]))
    p_lo = min(max(int(math.floor(-drift[0] + lo + 12)) - 1, 0), Z + 23)
    p_hi = min(max(int(math.floor(Z - 1 - drift[0] + hi + 12)) + 2, 0), Z + 23)
    Vp = (p_hi - p_lo + 1) * (X + 24) * (Y + 24)
    alg = V * im.itemsize * 2 + 3 * V * 4
    moves = {"spline_axis0": V * im.itemsize + 8 * Vp, "spline_axis1": 2 * 8 * Vp, "spline_axis2": 2 * 8 * Vp,
             "warp_cubic": 8 * Vp + 3 * V * 4 + V * im.itemsize}
    total_ms = sum(k_ms.values())
    gather_flop = 256 + 105          # float64 operations per output: the taps in SciPy's order + the cubic weights
    g_ms = k_ms.get("warp_cubic", 0.0)
    return {"workload": "cubic map_coordinates of one %dx%dx%d uint16 channel, drift + dense float32 field, resident" % (Z, X, Y),
            "ms_per_channel": round(sorted(ts)[len(ts) // 2] * 1e3, 3), "kernels_ms": k_ms,
            "roofline": {"bound": "hbm", "algorithmic_GB": round(alg / 1e9, 3), "achieved": round(alg / 1e9 / (total_ms * 1e-3), 1),
                         "peak": 8000.0, "unit": "GB/s", "frac": round(alg / 1e9 / (total_ms * 1e-3) / 8000.0, 4),
                         "padded_planes_computed": [p_lo, p_hi, Z + 24],
                         "prefilter_moves_GB": round(sum(moves.values()) / 1e9, 2),
                         "moved_GBps_by_kernel": {k: round(moves[k] / 1e9 / (k_ms[k] * 1e-3), 1) for k in k_ms if k in moves},
                         "gather": {"bound": "f64_valu", "f64_ops_per_output": gather_flop,
                                    "achieved": round(gather_flop * V / 1e12 / (g_ms * 1e-3), 2) if g_ms else None,
                                    "peak": 39.3, "unit": "Tinstr/s (non-fused float64 vector instructions)",
                                    "frac": round(gather_flop * V / 1e12 / (g_ms * 1e-3) / 39.3, 3) if g_ms else None},
                         "note": "exact float64 spline prefilter over the padded planes the gather can read "
                                 "(padded_planes_computed: first, last, of), each sample read once and written once per axis; "
                                 "the gather is bound by the float64 vector unit (SciPy's summation order fixes 256 "
                                 "operations per output)"}}


def _c5_runs(L, lib, movie):
    """Three movies from one host thread, then six on three host threads (callers: inside ONE stdout redirection)."""
    movie()
    n = 3
    L.check(lib.ia3_sync()); t0 = time.perf_counter()
    spots = 0
    for _ in range(n):
        k, drift = movie()
        spots += k
    dt = time.perf_counter() - t0
    # the reference runs one image per pool worker (field_of_view.py:1129-1142); here three movies at a time on three
    # host threads, each with its own streams: the upload and corrections of one overlap the fits of the others
    from concurrent.futures import ThreadPoolExecutor
    n_thr, n_par = 3, 6
    with ThreadPoolExecutor(max_workers=n_thr) as pool:
        list(pool.map(lambda _: movie(), range(n_thr)))
        t1 = time.perf_counter()
        outs = list(pool.map(lambda _: movie(), range(n_par)))
        dt_par = time.perf_counter() - t1
    return {"workload": "configs[4] on one GPU, per round-folder movie: 200-frame uint16 4-colour movie (host) -> upload -> "
                        "hot pixels, bleedthrough 3x3, illumination -> bead drift (phase correlation vs the resident reference "
                        "bead stack) -> cubic warp with drift + dense chromatic field -> seed + fit of 3 channels",
            "movies": n, "s_per_movie": round(dt / n, 4), "images_per_sec": round(3 * n / dt, 2),
            "spots_per_sec": round(spots / dt, 1), "drift": [round(float(x), 3) for x in drift],
            "three_host_threads": {"movies": n_par, "s_per_movie": round(dt_par / n_par, 4),
                                   "images_per_sec": round(3 * n_par / dt_par, 2),
                                   "spots_per_sec": round(sum(o[0] for o in outs) / dt_par, 1)}}




# ---------------------------------------------------------------------------------------------------------------------
# the boundary as the reference uses it: forked pool workers, one image per task
# ---------------------------------------------------------------------------------------------------------------------
_POOL_IMS = None   # host images of the forked-pool leg (inherited through fork, not pickled)


def _pool_init():
    """Every worker opens the GPU itself (HIP state does not survive fork) and makes one small call, so that the timed
    tasks do not pay for the library load and the first allocations."""
    from imageanalysis3_amd import synth
    from imageanalysis3_amd.spot_tools.fitting import fit_fov_image
    im = synth.make_fov((30, 128, 128), 50, 1, dtype=np.uint16)[0]
    fit_fov_image(im, "647", th_seed=TH_SEED, max_num_seeds=None, verbose=False)


def _pool_task(k):
    from imageanalysis3_amd.spot_tools.fitting import fit_fov_image
    im = _POOL_IMS[k % len(_POOL_IMS)]
    t0 = time.perf_counter()
    t = fit_fov_image(im, "647", th_seed=TH_SEED, max_num_seeds=None, verbose=False)
    return len(t), time.perf_counter() - t0


def forked_pool_leg(ims, workers=6, tasks=48):
    """The drop-in pattern of classes/field_of_view.py:1129-1138: mp.Pool workers (forked BEFORE this process touches the
    GPU), each calling fit_fov_image(host uint16 ndarray) on one image per task, chunksize=1.  Six workers: the GPU boxes
    of this pool admit six processes on the card."""
    global _POOL_IMS
    import multiprocessing as mp
    _POOL_IMS = [ims[0], ims[1], ims[2], np.ascontiguousarray(ims[0][:, ::-1]), np.ascontiguousarray(ims[1][:, :, ::-1]),
                 np.ascontiguousarray(ims[2][::-1])]
    with mp.get_context("fork").Pool(workers, initializer=_pool_init) as pool:
        pool.map(_pool_task, range(workers), chunksize=1)     # every worker has made a full-size call
        t0 = time.perf_counter()
        res = pool.map(_pool_task, range(tasks), chunksize=1)
        dt = time.perf_counter() - t0
    _POOL_IMS = None
    per = sorted(r[1] for r in res)
    return {"workload": "%d forked workers, fit_fov_image(host uint16 2048x2048x50 ndarray) per task, chunksize=1, %d tasks over 6 "
                        "different images" % (workers, tasks),
            "workers": workers, "tasks": tasks, "fovs_per_sec": round(tasks / dt, 2), "ms_per_fov": round(dt / tasks * 1e3, 2),
            "spots_per_sec": round(sum(r[0] for r in res) / dt, 1),
            "call_ms": {"min": round(per[0] * 1e3, 1), "median": round(per[len(per) // 2] * 1e3, 1), "max": round(per[-1] * 1e3, 1)},
            "note": "every task uploads its image (419 MB), seeds and fits it alone on its process's own stream and returns "
                    "the table; batch_entry_fovs_per_sec = the same kind of images through ia3_fit_fovs from one process "
                    "(streaming.u16)"}


_CPU_IM = None   # the FOV the CPU-baseline workers cut their windows from (inherited through fork, not pickled)


def _cpu_run(args):
    """One oracle pass over the window [x0:x0+c, y0:y0+c] of _CPU_IM (module level: runs in forked workers too)."""
    x0, y0, c, th = args
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import np_oracle as O
    sub = np.ascontiguousarray(_CPU_IM[:, x0:x0 + c, y0:y0 + c])
    t0 = time.perf_counter()
    t = O.fit_fov_image(sub, "647", th_seed=th, max_num_seeds=None)
    return len(t), time.perf_counter() - t0


def cpu_baseline(im, crop):
    """The oracle (NumPy/SciPy restatement of the reference's CPU path: ndimage-exact filters, MINPACK lmder through
    scipy.optimize.leastsq, cKDTree Voronoi cells, Python loop over seeds — same structure and cost profile as the
    reference) on the WHOLE first FOV from one process: no extrapolation (crop > 0 restricts it to a window, for quick
    runs).  `all_cores` then runs one worker process per host core at once, each on a DIFFERENT window of the FOV sized
    for ~15 s — the way the reference parallelises (one image per process, classes/field_of_view.py:1129-1138)."""
    global _CPU_IM
    _CPU_IM = im
    side = min(im.shape[1], im.shape[2])
    whole = crop <= 0 or crop >= side
    if whole:
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import np_oracle as O
        t0 = time.perf_counter()
        t = O.fit_fov_image(im, "647", th_seed=TH_SEED, max_num_seeds=None)
        dt = time.perf_counter() - t0
        n, frac = len(t), 1.0
        sample = "oracle fit_fov_image on the whole first FOV (%d x %d x %d, %s), one process" % (im.shape + (im.dtype.name,))
    else:
        n, dt = _cpu_run((0, 0, crop, TH_SEED))
        frac = (crop * crop) / float(im.shape[1] * im.shape[2])
        sample = "oracle fit_fov_image on the [0:%d, 0:%d, 0:%d] window of the first FOV (%.1f%% of the voxels)" % (
            im.shape[0], crop, crop, 100.0 * frac)
    out = {"value": round(n / dt, 2), "unit": "spots/s", "cores": 1, "kind": "port",
           "fovs_per_sec": round(frac / dt, 5), "seconds": round(dt, 1), "spots": int(n), "sample": sample}
    try:
        import multiprocessing as mp
        ncore = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
        ncore = max(1, min(ncore, 16))   # a 1-GPU box gives this job a 16-core share
        if ncore > 1:
            # a window that takes one worker ~15 s at the single-core rate just measured (cost ~ voxels)
            wc = int(min(side, max(128, side * (15.0 / max(dt / frac, 1e-3)) ** 0.5))) // 32 * 32
            wfrac = (wc * wc) / float(im.shape[1] * im.shape[2])
            per = max(1, (im.shape[1] - wc) // max(1, int(ncore ** 0.5)))
            wins = []
            for k in range(ncore):   # worker k gets the window at a different offset (wrapping grid of window origins)
                x0 = (k * per) % max(1, im.shape[1] - wc + 1)
                y0 = ((k * 7 + 3) * per) % max(1, im.shape[2] - wc + 1)
                wins.append((x0, y0, wc, TH_SEED))
            t0 = time.perf_counter()
            with mp.get_context("fork").Pool(ncore) as pool:
                res = pool.map(_cpu_run, wins)
            wall = time.perf_counter() - t0
            out["all_cores"] = {"value": round(sum(r[0] for r in res) / wall, 2), "unit": "spots/s", "cores": ncore,
                                "fovs_per_sec": round(ncore * wfrac / wall, 5), "seconds": round(wall, 1),
                                "sample": "%d worker processes at once, each on a different %dx%d window of the FOV" % (ncore, wc, wc)}
    except Exception as e:   # the single-core figure is the contract; the pool is extra
        out["all_cores"] = {"error": str(e)}
    return out


if __name__ == "__main__":
    main()
