"""Fixtures of the chromosomal spot scores: tests/golden/scoring.npz.

Loads the reference's own ``spot_tools/scoring.py`` by file (it imports ``_distance_zxy`` from its parent package, so a stub
parent holding that constant is registered first; the ``np.int`` / ``np.float`` aliases it uses are put back) and runs it on
the calls of tests/harness/scoring_cases.py::fixture_calls.  Only outputs are stored: ``<key>__<i>`` is output i of the call
``key`` (an exception of the reference is stored as its text), ``sig_<name>`` is str(inspect.signature) of a reference
function.

Needs the reference tree (IA3_REFERENCE); nothing here runs on the GPU.

    python scripts/make_scoring_golden.py

The script asserts the facts about the reference's arithmetic that csrc/ia3_score.h and score.hip are built on.
"""
import importlib.util
import inspect
import io
import os
import sys
import types
import warnings
from contextlib import redirect_stdout
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

REF = os.environ.get("IA3_REFERENCE", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden", "scoring.npz")


def load_reference():
    for n, t in (("int", int), ("bool", bool), ("float", float)):   # removed in numpy >= 1.24
        if not hasattr(np, n):
            setattr(np, n, t)
    parent = types.ModuleType("ia3_ref_spot_tools")
    parent.__path__ = []
    parent._distance_zxy = [200, 108, 108]
    sys.modules["ia3_ref_spot_tools"] = parent
    spec = importlib.util.spec_from_file_location("ia3_ref_spot_tools.scoring", os.path.join(REF, "spot_tools", "scoring.py"))
    m = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = m
    spec.loader.exec_module(m)
    return m


def _fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def check_facts(ref):
    """What the kernels rest on, asserted on NumPy and on the reference itself."""
    from harness import scoring_cases as K
    rng = np.random.default_rng(3)
    # np.nanmean(x, axis=0) of (m, 3): one accumulator per column, row after row, NaN as 0, one count per column
    x = rng.normal(size=(200, 3)) * 1000.
    x[rng.random(x.shape) < 0.1] = np.nan
    acc, cnt = np.zeros(3), np.zeros(3)
    for r, row in enumerate(x):
        v = np.where(np.isnan(row), 0., row)
        acc = v if r == 0 else acc + v
        cnt += ~np.isnan(row)
    assert K.same(np.nanmean(x, axis=0), acc / cnt)
    pair = np.array([np.add.reduce(np.ascontiguousarray(np.where(np.isnan(x[:, k]), 0., x[:, k]))) for k in range(3)]) / cnt
    assert not K.same(pair, acc / cnt)                      # ... which is not the pairwise order of a contiguous axis
    # np.linalg.norm(x, axis=1): sqrt((a*a + b*b) + c*c), no fused multiply-add
    y = rng.normal(size=(5000, 3)) * 300.
    assert K.same(np.linalg.norm(y, axis=1), np.sqrt((y[:, 0] * y[:, 0] + y[:, 1] * y[:, 1]) + y[:, 2] * y[:, 2]))
    # np.linalg.norm(v) of one vector is sqrt(v.dot(v)), BLAS's dot: fma(c, c, fma(b, b, a*a)) on this OpenBLAS
    fused = np.array([np.sqrt(_fma(c, c, _fma(b, b, a * a))) for a, b, c in y[:2000].tolist()])
    assert K.same(np.array([np.linalg.norm(v) for v in y[:2000]]), fused)
    assert not K.same(fused, np.linalg.norm(y[:2000], axis=1))
    # _local_distance: the rows of ids id-half .. id+half without id, ascending, each id's rows in row order, through the
    # column accumulators above; the last norm is the one-vector form
    sel_ids = np.array([4, 2, 3, 2, 6, 1, 3, 3, 0])
    sel = rng.normal(size=(9, 3)) * 500.
    spot = rng.normal(size=3) * 500.
    rows = [sel[k] for i in (1, 2, 4, 5) for k in np.where(sel_ids == i)[0]]
    acc = rows[0]
    for row in rows[1:]:
        acc = acc + row
    d = acc / len(rows) - spot
    want = np.sqrt(_fma(d[2], d[2], _fma(d[1], d[1], d[0] * d[0])))
    assert K.same(ref._local_distance([spot], [3], sel, sel_ids, local_size=5), [want])
    assert K.same(ref._local_distance([spot], [3], sel, sel_ids, local_size=6), [want])          # int((6 - 1) / 2) == 2
    assert np.isnan(ref._local_distance([spot], [3], sel, sel_ids, local_size=2)).all()          # half 0: nothing gathered
    assert np.isnan(ref._local_distance([spot], [9], sel, sel_ids, local_size=5)).all()          # ids 7, 8, 10, 11: none
    # a row with one NaN coordinate still feeds the other columns; all rows with a NaN: invalid
    sel2 = sel.copy()
    sel2[1, 0] = np.nan                                                                           # one of the rows of id 2
    got = ref._local_distance([spot], [3], sel2, sel_ids, local_size=3)                           # ids 2 and 4: rows 1, 3, 0
    m = np.array([(0. + sel2[3, 0] + sel2[0, 0]) / 2., (sel2[1, 1] + sel2[3, 1] + sel2[0, 1]) / 3., (sel2[1, 2] + sel2[3, 2] + sel2[0, 2]) / 3.]) - spot
    assert K.same(got, [np.sqrt(_fma(m[2], m[2], _fma(m[1], m[1], m[0] * m[0])))])
    sel3 = sel.copy()
    sel3[[0, 1, 3], 1] = np.nan
    assert K.same(ref._local_distance([spot], [3], sel3, sel_ids, local_size=3, invalid_dist=-5.), [-5.])
    # neighboring_distances: both sides only when id + step is present; the reverse side is not tested
    z = rng.normal(size=(6, 3)) * 400.
    ids = np.array([0, 1, 1, 3, 5, 5])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fwd, rev = ref.neighboring_distances(z, ids, invalid_dist=-1.)
    assert fwd[0] == np.median(np.linalg.norm(z[1:3] - z[0], axis=1)) and np.isnan(rev[0])      # np.nanmedian([]) is NaN
    assert (fwd[1:] == -1.).all() and (rev[1:] == -1.).all()                                     # id 3 has a reverse region only
    assert K.same(np.nanmean([np.array([1., np.nan, np.nan]), np.array([4., 2., np.nan])], axis=0), [(1. + 4.) / 2, 2., np.nan])
    # _cum_prob: `<=` counts over n, min_p / max_p, the clamps last
    data = np.array([0., 0., 1., 2., 2., 3., np.nan, 7.])
    n = 7
    for vmin, vmax in ((-np.inf, np.inf), (0, 2), (2, 2), (3, 1), (9, 12)):
        t = np.array([-1., 0., 1.5, 2., 7., 8., np.nan])
        c = np.array([(data[:6].tolist() + [7.] <= np.float64(np.inf if np.isnan(v) else v)).sum() for v in t]) / n
        lo, hi = (np.array(data[~np.isnan(data)]) <= vmin).sum() / n, (np.array(data[~np.isnan(data)]) <= vmax).sum() / n
        want = (c - lo) if hi <= lo else (c - lo) / (hi - lo)
        want[want <= 0] = 0
        want[want >= 1] = 1
        assert K.same(ref._cum_prob(data, t, vmin=vmin, vmax=vmax), want), (vmin, vmax)
    # np.nanmean of a contiguous 1-D array: NaN as 0 in the pairwise sum, the count of the others below it
    v = rng.normal(size=1000) * 100.
    v[rng.random(1000) < 0.2] = np.nan
    assert K.same(np.nanmean(v), np.add.reduce(np.where(np.isnan(v), 0., v)) / (~np.isnan(v)).sum())
    # the package's default distance_zxy is a list, which generate_ref_from_chromosome refuses
    sel4 = np.concatenate([np.ones((9, 1)), sel], axis=1)
    try:
        ref.generate_ref_from_chromosome(sel4)
        raise AssertionError("a list was accepted")
    except TypeError:
        pass
    # the fallbacks and their types
    sel4[:, 1:] = np.nan
    sel4[:, 0] = 0.
    with warnings.catch_warnings(), redirect_stdout(io.StringIO()):
        warnings.simplefilter("ignore")
        r = ref.generate_ref_from_chromosome(sel4, distance_zxy=K.DZXY, ref_dist_metric='cdf')
    assert r[0] == [1000] and r[1] == [np.inf] and r[2] == [np.inf] and type(r[0]) is list and isinstance(r[3], np.ndarray) and r[3].tolist() == [1.]
    assert isinstance(ref.radius_of_gyration(np.zeros(3)), IndexError)


def main():
    from harness import scoring_cases as K
    warnings.filterwarnings("ignore")
    ref = load_reference()
    check_facts(ref)
    out = {}
    with np.errstate(all="ignore"), redirect_stdout(io.StringIO()):
        for key, f in K.fixture_calls():
            for i, a in enumerate(f(ref)):
                out["%s__%d" % (key, i)] = a
    for name in K.SIGNATURE_NAMES:
        out["sig_" + name] = np.array(str(inspect.signature(getattr(ref, name))))
    np.savez_compressed(OUT, **out)
    floats = [v for v in out.values() if v.dtype == np.float64]
    texts = sorted(set(str(v).split(":")[0] for v in out.values() if v.dtype.kind == 'U' and ":" in str(v)))
    print("wrote %s: %d keys, %d bytes, %d NaN, %d inf, raised: %s" % (OUT, len(out), os.path.getsize(OUT), sum(int(np.isnan(v).sum()) for v in floats),
                                                                      sum(int(np.isinf(v).sum()) for v in floats), texts))


if __name__ == "__main__":
    main()
