"""Where the time of the per-cell pickers goes: profiles/cell_picking.json.

The workload is N cells x R regions x 5 candidates per chromosome and region, 'linear' scores, at C = 2 and C = 3 chromosomes
(--cells 2000 --regions 1000 is the full shape).  On the device it reports the upload (packing on the host and the copy),
the merge kernel, one forward pass, one whole EM iteration with its parts (host bookkeeping before, E-step, forward pass,
host bookkeeping after) and the full EM with its final check; kernel times are the library's own event timings.

    python scripts/time_cell_picking.py --cells 2000 --regions 1000            # on the GPU
    python scripts/time_cell_picking.py --reference --cells 20 --regions 1000  # the reference's procedure on one core

``--reference`` runs the reference's own functions (IA3_REFERENCE names its tree) on 1/100 of the cells and adds its
seconds to the same file; the two runs are merged by key.
"""
import argparse
import io
import json
import os
import sys
import time
from contextlib import redirect_stdout

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

DZXY = np.array([200., 108., 108.])
OUT = os.path.join(ROOT, "profiles", "cell_picking.json")


def make_cells(n_cells, R, C, n_cand, seed=7):
    """Cells of R regions (ids 0 .. R-1) whose C chromosomes walk 30 pixels apart, n_cand candidates of 11 columns each."""
    rng = np.random.default_rng(seed)
    cells = []
    for k in range(n_cells):
        centers = np.array([[10. + 2 * c, 200. + 30. * c, 300. + 30. * (c % 2)] for c in range(C)])
        walk = centers[None] + np.cumsum(rng.normal(size=(R, C, 3)) * np.array([0.3, 1.5, 1.5]), axis=0)
        t = np.abs(rng.normal(size=(R, C, n_cand, 11))) + 0.5
        t[..., 0] = np.exp(rng.normal(size=(R, C, n_cand))) * 2.
        t[..., 1:4] = walk[:, :, None, :] + rng.normal(size=(R, C, n_cand, 3)) * np.array([0.4, 1.5, 1.5])
        cells.append(([[t[r, c] for c in range(C)] for r in range(R)], np.arange(R), [centers[c] for c in range(C)]))
    return cells


def time_device(n_cells, R, C, n_cand, num_iters):
    from imageanalysis3_amd import _lib as L
    from imageanalysis3_amd.spot_tools import picking as P
    res = dict(cells=n_cells, regions=R, chromosomes=C, candidates=n_cand)
    t = time.time()
    cells = make_cells(n_cells, R, C, n_cand)
    res["make_workload_s"] = time.time() - t
    t0 = time.time()
    say = lambda what: print("  C=%d %s at %.0f s" % (C, what, time.time() - t0), flush=True)    # noqa: E731
    L.profile_enable(True)
    L.profile_collect()
    t = time.time()
    pop = P._upload_cells(cells, DZXY)
    res["upload_s"] = time.time() - t
    say("uploaded")
    t = time.time()
    P._merge(pop, 0., True)
    res["merge_call_s"] = time.time() - t
    res["merge_kernel_ms"] = L.profile_collect().get("cellpick_merge", (0, 0.))[1]
    t = time.time()
    pop._rows4 = pop.merged_rows4()
    res["merged_rows_host_s"] = time.time() - t
    Pm = P._dynamic_params('median', 100, 0., 'linear', 5, 2, 1, 1, 2, True, 0., -1000., False, False, DZXY, [0, 3000], False)
    Pm["timings"] = {}
    t = time.time()
    with redirect_stdout(io.StringIO()):
        P._dynamic_cells(pop, list(range(n_cells)), {}, {}, None, None, Pm)
    res["one_iteration_s"] = time.time() - t
    say("one iteration done")
    res["one_iteration_parts_s"] = dict(Pm["timings"])
    prof = L.profile_collect()
    res["forward_kernel_ms"] = prof.get("cellpick_forward", (0, 0.))[1]
    res["e_step_kernels_ms"] = {k: v[1] for k, v in prof.items() if k.startswith("score_")}
    P._close_cells(pop)
    tm = {}
    t = time.time()
    with redirect_stdout(io.StringIO()), np.errstate(all="ignore"):
        out = P.population_EM_pick_spots(cells, num_iters=num_iters, distance_zxy=DZXY, return_indices=True, verbose=False, timings=tm)
    res["full_em_s"] = time.time() - t
    res["full_em_parts_s"] = {k: (v if not isinstance(v, list) else [round(x, 4) for x in v]) for k, v in tm.items()}
    res["full_em_iterations"] = len(tm["iterations_s"])
    res["full_em_forward_kernel_ms"] = L.profile_collect().get("cellpick_forward", (0, 0.))[1]
    assert len(out) == n_cells
    return res


def time_reference(n_cells, R, C, n_cand, num_iters):
    import make_cell_picking_golden as G
    mods = G.load_reference()
    P = mods["picking"]
    res = dict(cells=n_cells, regions=R, chromosomes=C, candidates=n_cand, cores=1)
    cells = make_cells(n_cells, R, C, n_cand)
    with redirect_stdout(io.StringIO()), np.errstate(all="ignore"):
        t = time.time()
        for cand, ids, coords in cells:
            [P.merge_spot_list(lists, append_nan_spots=True, chrom_coords=coords) for lists in cand]
        res["merge_s"] = time.time() - t
        t = time.time()
        for cand, ids, coords in cells:
            P.dynamic_pick_spots_for_chromosomes(cand, ids, coords, distance_zxy=DZXY, distance_limits=[0, 3000], verbose=False)
        res["one_iteration_s"] = time.time() - t
        t = time.time()
        for cand, ids, coords in cells:
            P.EM_pick_spots_for_chromosomes(cand, ids, coords, num_iters=num_iters, distance_zxy=DZXY, return_indices=True, verbose=False)
        res["full_em_s"] = time.time() - t
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=2000)
    ap.add_argument("--regions", type=int, default=1000)
    ap.add_argument("--candidates", type=int, default=5)
    ap.add_argument("--chromosomes", type=int, nargs="+", default=[2, 3])
    ap.add_argument("--num-iters", type=int, default=10)
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    doc = json.load(open(a.out)) if os.path.isfile(a.out) else {}
    for C in a.chromosomes:
        key = "%s_C%d" % ("reference" if a.reference else "device", C)
        f = time_reference if a.reference else time_device
        doc[key] = f(a.cells, a.regions, C, a.candidates, a.num_iters)
        print(key, json.dumps(doc[key]))
        with open(a.out, "w") as fh:
            json.dump(doc, fh, indent=1, sort_keys=True)
            fh.write("\n")


if __name__ == "__main__":
    main()
