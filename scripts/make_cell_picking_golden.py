"""Fixtures of the per-cell spot pickers: tests/golden/cell_picking.npz.

Loads the reference's own ``spot_tools/picking.py``, ``scoring.py`` and ``checking.py`` by file, behind stub parent packages
that hold the constants and sibling modules they import (the ``np.int`` / ``np.bool`` / ``np.float`` aliases they use are
put back), and runs them on the calls of tests/harness/cell_picking_cases.py::fixture_calls.  Only outputs are stored:
``<key>__<i>`` is output i of the call ``key`` (an exception of the reference is stored as its text), ``sig_<name>`` is
str(inspect.signature) of a reference function, ``flag_<key>`` the tie flag below and ``tr_<key>_*`` what the reference's
dynamic picker held when it returned (merged rows of the regions it walked, their scores, dynamic scores, pointers and
neighbour references), which the stand-alone check of csrc/ia3_cellpick.h replays.

THE TIE RULE.  ``np.argsort``'s default kind is not stable: on tied keys its order depends on the host's CPU (with AVX-512
dispatch it differs from ``kind='stable'`` even at length 4), and so does the reference's output.  Every case is run twice:
as the reference stands, and with ``np.argsort`` patched in this process so that its default kind is 'stable' (ascending
index among equal keys, NaN last), which is the device's rule.  The fixture stores the second run -- still the reference's
program, with only the tie order pinned -- and ``flag_<key>``: whether the first run gave the same outputs.  Every 'linear'
case must carry a true flag (asserted here); 'cdf' cases tie on -inf and are compared against the pinned run only.

Needs the reference tree (IA3_REFERENCE); nothing here runs on the GPU.

    python scripts/make_cell_picking_golden.py

The script asserts the facts about NumPy's and the reference's arithmetic that csrc/ia3_cellpick.h is built on.
"""
import importlib.util
import inspect
import io
import itertools
import os
import sys
import types
import warnings
from contextlib import redirect_stdout

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

REF = os.environ.get("IA3_REFERENCE", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden", "cell_picking.npz")
_ARGSORT = np.argsort


def load_reference():
    for n, t in (("int", int), ("bool", bool), ("float", float)):   # removed in numpy >= 1.24
        if not hasattr(np, n):
            setattr(np, n, t)
    top = types.ModuleType("ia3_ref")
    top.__path__ = []
    for name in ("get_img_info", "corrections", "visual_tools"):
        setattr(top, name, types.ModuleType("ia3_ref." + name))
        sys.modules["ia3_ref." + name] = getattr(top, name)
    sys.modules["ia3_ref"] = top
    parent = types.ModuleType("ia3_ref.spot_tools")
    parent.__path__ = []
    parent._distance_zxy = [200, 108, 108]
    parent._sigma_zxy = [1.35, 1.9, 1.9]
    parent._correction_folder = parent._temp_folder = ""
    sys.modules["ia3_ref.spot_tools"] = parent
    mods = {}
    for name in ("scoring", "checking", "picking"):
        spec = importlib.util.spec_from_file_location("ia3_ref.spot_tools." + name, os.path.join(REF, "spot_tools", name + ".py"))
        m = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = m
        setattr(parent, name, m)
        spec.loader.exec_module(m)
        mods[name] = m
    return mods


def stable_argsort(a, axis=-1, kind=None, order=None, **kw):
    return _ARGSORT(a, axis=axis, kind='stable' if kind is None else kind, order=order, **kw)


def check_facts(mods):
    """What the kernels rest on, asserted on NumPy and on the reference itself."""
    from harness import cell_picking_cases as K
    rng = np.random.default_rng(4)
    # np.linalg.norm(x, axis=1): sqrt((a*a + b*b) + c*c), no fused multiply-add; SciPy's cdist has the same arithmetic
    y = rng.normal(size=(5000, 3)) * 300.
    assert K.same(np.linalg.norm(y, axis=1), np.sqrt((y[:, 0] * y[:, 0] + y[:, 1] * y[:, 1]) + y[:, 2] * y[:, 2]))
    from scipy.spatial.distance import cdist
    a, b = y[:70], y[70:150]
    d = a[:, None, :] - b[None, :, :]
    assert K.same(cdist(a, b), np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]))
    # np.nansum of a list of fewer than 8 numbers: a plain left-to-right sum with NaN counted as 0
    for C in range(1, 8):
        v = rng.normal(size=(4000, C)) * np.exp(rng.normal(size=(4000, C)) * 4.)
        v[rng.random(v.shape) < 0.1] = np.nan
        want = np.where(np.isnan(v[:, 0]), 0., v[:, 0])
        for k in range(1, C):
            want = want + np.where(np.isnan(v[:, k]), 0., v[:, k])
        assert K.same(np.array([np.nansum([row[k] for k in range(C)]) for row in v]), want), C
    # itertools.product: the last position varies fastest
    assert list(itertools.product([4, 5], [7, 8, 9]))[:4] == [(4, 7), (4, 8), (4, 9), (5, 7)]
    assert list(itertools.product(np.arange(2), repeat=2)) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    # argsort(scores)[-C:]: the C largest, ascending; the pinned order takes equal keys by ascending index, NaN last
    s = np.array([3., np.nan, 1., 3., -np.inf, np.nan, 1.])
    assert stable_argsort(s).tolist() == [4, 2, 6, 0, 3, 1, 5] and stable_argsort(s)[-3:].tolist() == [3, 1, 5]
    # the first-maximum rules: np.argmax and np.argmin take the first extreme, a NaN before any number
    assert np.argmax([1., 5., 5.]) == 1 and np.argmax([1., np.nan, 9., np.nan]) == 1
    assert np.argmin([3., 1., 1.]) == 1 and np.argmin([3., np.nan, 0., np.nan]) == 1
    t = np.array([2., 7., 7., 1., 7.])
    sids = np.where(t == np.nanmax(t))[0]
    assert sids.tolist() == [1, 2, 4] and sids[np.argmax(np.array([5, 9, 9]))] == 2
    # the reference's helpers on lists without ties
    P = mods["picking"]
    assert P._all_score_combinations([np.zeros(2), np.zeros(2)]) == [(0, 1), (1, 0)]
    assert P._optimized_score_combinations([np.array([1., 5., 3., 0.]), np.array([9., 8., 7., 6.])]) == [(2, 1), (2, 0), (1, 0)]
    assert P._optimized_score_combinations([np.array([1., 5., 3.]), np.full(3, -np.inf)], chrom_share_spots=True)[:4] == [(2, 0), (2, 1), (2, 2), (1, 0)]
    # a kept spot drops its close neighbours, a dropped one drops nothing (:727-742), and np.argmin's first minimum owns it
    z = np.zeros((3, 11))
    z[:, 0] = 5.
    z[:, 2] = [0., 0.08, 0.16]
    got = P.merge_spot_list([z[:2], z[2:]], append_nan_spots=True, chrom_coords=[np.zeros(3), np.zeros(3)])
    assert len(got) == 3 and got[0, 2] == 0. and got[1, 2] == 0.16 and got[2, 0] == 0. and np.isnan(got[2, 4:]).all()


def trace_dynamic(mods, f, ns):
    """Run ``f(ns)`` (one dynamic call) and return what the reference's dynamic picker held at its return."""
    S, P = mods["scoring"], mods["picking"]
    scores, held = [], {}
    real = S.spot_score_in_chromosome

    def record(*a, **k):
        r = real(*a, **k)
        scores.append(np.array(r, dtype=np.float64).copy())
        return r

    def prof(frame, event, arg):
        if event == "return" and frame.f_code.co_name == "dynamic_pick_spots_for_chromosomes" and "_dy_pointer_list" in frame.f_locals:
            held.update({k: frame.f_locals[k] for k in ("_dy_pointer_list", "_dy_score_list", "_ids", "_id_indices", "nb_dist_list",
                                                        "_merged_spot_list", "_num_chroms")})
    S.spot_score_in_chromosome = record
    sys.setprofile(prof)
    try:
        f(ns)
    finally:
        sys.setprofile(None)
        S.spot_score_in_chromosome = real
    C, idx = held["_num_chroms"], held["_id_indices"]
    R = len(held["_merged_spot_list"])
    assert len(scores) == C * R
    out = dict(ids=np.array(held["_ids"], dtype=np.int64), idx=np.array(idx, dtype=np.int64),
               K=np.array([len(held["_merged_spot_list"][i]) for i in idx], dtype=np.int64))
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dtype=dt)    # noqa: E731
    out["rows"] = cat([held["_merged_spot_list"][i][:, :4] for i in idx], np.float64).reshape(-1, 4)
    out["score"] = np.array([cat([scores[c * R + i] for i in idx], np.float64) for c in range(C)])
    out["dy"] = np.array([cat(held["_dy_score_list"][c], np.float64) for c in range(C)])
    out["ptr"] = np.array([cat(held["_dy_pointer_list"][c], np.int16) for c in range(C)])
    for c in range(C):
        out["nb_%d" % c] = np.atleast_1d(np.array(held["nb_dist_list"][c], dtype=np.float64))
    return out


def main():
    from harness import cell_picking_cases as K
    warnings.filterwarnings("ignore")
    mods = load_reference()
    ns = K.namespace(mods["picking"], mods["checking"])
    check_facts(mods)
    out, flags = {}, {}
    with np.errstate(all="ignore"), redirect_stdout(io.StringIO()):
        for key, f in K.fixture_calls():
            first = f(ns)
            np.argsort = stable_argsort
            try:
                pinned = f(ns)
            finally:
                np.argsort = _ARGSORT
            flags[key] = len(first) == len(pinned) and all(K.same(a, b) for a, b in zip(first, pinned))
            for i, a in enumerate(pinned):
                out["%s__%d" % (key, i)] = a
            out["flag_" + key] = np.array(flags[key])
        calls = dict(K.fixture_calls())
        np.argsort = stable_argsort
        try:
            for key in K.TRACED:
                cellname, kw = [(c, kw) for k, c, kw in K.DYNAMIC_CASES if k == key][0]

                def f(ns, cellname=cellname, kw=kw):
                    cand, ids, coords = K.cell(cellname)
                    return ns.picking.dynamic_pick_spots_for_chromosomes(cand, ids, coords, return_indices=True, **K.dynamic_kwargs(kw))
                for name, a in trace_dynamic(mods, f, ns).items():
                    out["tr_%s_%s" % (key, name)] = a
        finally:
            np.argsort = _ARGSORT
    bad = [k for k in K.LINEAR_KEYS if not flags[k]]
    assert not bad, "'linear' cases whose output depends on the order of tied keys: %s" % bad
    for name in K.SIGNATURE_NAMES:
        out["sig_" + name] = np.array(str(inspect.signature(getattr(mods["picking"], name))))
    for name in K.CHECKING_SIGNATURE_NAMES:
        out["sig_" + name] = np.array(str(inspect.signature(getattr(mods["checking"], name))))
    np.savez_compressed(OUT, **out)
    texts = sorted(set(str(v) for v in out.values() if v.dtype.kind == 'U' and ":" in str(v) and not str(v).startswith("(")))
    print("wrote %s: %d keys, %d bytes; order-dependent: %s" % (OUT, len(out), os.path.getsize(OUT), [k for k, v in flags.items() if not v]))
    for t in texts:
        print("  raised:", t[:150])
    assert calls


if __name__ == "__main__":
    main()
