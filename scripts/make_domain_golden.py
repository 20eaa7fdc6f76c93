"""Fixtures of the domain distances: tests/golden/domain_distances.npz.

Loads the reference's own ``domain_tools/distance.py`` by file (it needs numpy, scipy and matplotlib only; the ``np.int`` /
``np.float`` aliases it uses are put back the way oracle/ref_loader.py does) and runs it on the calls of
tests/harness/domain_cases.py::fixture_calls.  Only outputs are stored, under the keys of that list:

    win_<population>_<metric>        _sliding_window_dist, (N, len(WDS), R) float64
    pd_<source>_<metric>_<allow>_<raw|norm>   domain_pdists of every copy, (N, 15) float64
    nb_<source>_<use_local>_<min_dom_sz>_<raw|norm>   domain_neighboring_dists of every copy, (N, 5) float64
    dd_<source>_values / _intzero    single domain_distance calls and whether each returned Python's integer 0
    cf_<source>_<threshold>_<a|b>    _domain_contact_freq of every copy, (N, D, D) float64
    sig_<name>                       str(inspect.signature) of the five reference functions

Needs the reference tree (IA3_REFERENCE); nothing here runs on the GPU.

    python scripts/make_domain_golden.py

The script asserts the facts about the reference's arithmetic that csrc/ia3_domain.h and domain.hip are built on.
"""
import importlib.util
import inspect
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

REF = os.environ.get("IA3_REFERENCE", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden", "domain_distances.npz")


def load_reference():
    import matplotlib
    matplotlib.use("Agg")
    for n, t in (("int", int), ("bool", bool), ("float", float)):   # removed in numpy >= 1.24
        if not hasattr(np, n):
            setattr(np, n, t)
    spec = importlib.util.spec_from_file_location("ia3_ref_domain_distance", os.path.join(REF, "domain_tools", "distance.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def check_facts(ref):
    """What the kernels rest on, asserted on the reference itself."""
    from scipy.spatial.distance import pdist, squareform
    from harness import domain_cases as K
    # the harness's distance map is scipy's squareform(pdist(.)), NaN loci included
    for pop in list(K.window_populations().values()) + list(K.domain_populations().values()):
        for z in pop:
            assert K.same(K.distance_map(z), squareform(pdist(z)))
    # set order: a map whose entries name their own place shows in 'mean' which entries are added in which order
    R, i, wd = 12, 6, 3
    mat = np.arange(R * R, dtype=np.float64).reshape(R, R) * 1.0000001 + 1.
    left = [mat[r, c] for r in range(i - wd, i) for c in range(r + 1, i)]
    right = [mat[r, c] for r in range(i, i + wd) for c in range(r + 1, i + wd)]
    inter = [mat[r, c] for r in range(i - wd, i) for c in range(i, i + wd)]
    intra = np.array(left + right)
    inter = np.array(inter)
    want = (np.mean(inter) - np.mean(intra)) / np.sqrt(np.var(inter) + np.var(intra))
    assert K.same(ref._sliding_window_dist(mat, wd, 'mean')[i], want)
    # `> 0` filters the intra set only: a zero between the windows is kept, a zero inside one is dropped
    m2 = mat.copy()
    m2[i - 1, i] = 0.
    inter2 = np.array([m2[r, c] for r in range(i - wd, i) for c in range(i, i + wd)])
    assert K.same(ref._sliding_window_dist(m2, wd, 'insulation')[i], np.mean(inter2) / np.mean(intra))
    m3 = mat.copy()
    m3[i - 2, i - 1] = 0.
    intra3 = np.array([v for v in [m3[r, c] for r in range(i - wd, i) for c in range(r + 1, i)] if v > 0] + right)
    assert len(intra3) == len(intra) - 1
    assert K.same(ref._sliding_window_dist(m3, wd, 'insulation')[i], np.mean(inter) / np.mean(intra3))
    # [i, j] is read, not [j, i]: the lower triangle of a diagonal block never enters
    m4 = mat.copy()
    m4[i - 1, i - 2] = -77.
    assert K.same(ref._sliding_window_dist(m4, wd, 'mean'), ref._sliding_window_dist(mat, wd, 'mean'))
    # domain_distance keeps zeros in the intra set
    z = K.domain_populations()["lattice"][0]
    assert (pdist(z[3:70]) == 0).any()
    # the integer 0 returns
    assert type(ref.domain_distance(z, (5, 5), (10, 20))) is int
    assert type(ref.domain_distance(z, (0, 1), (1, 2))) is int          # two one-locus domains: no intra distance
    r = ref.domain_distance(z, (3, 70), (71, 135), _metric='absolute_median', _allow_minus_distance=False)
    f = ref.domain_distance(z, (3, 70), (71, 135), _metric='absolute_median', _allow_minus_distance=True)
    assert (type(r) is int and r == 0) if 0 > f else K.same(r, f)
    assert type(ref.domain_distance(z, (71, 135), (3, 10), _metric='absolute_median', _allow_minus_distance=False)) in (int, np.float64)


def main():
    from harness import domain_cases as K
    warnings.filterwarnings("ignore")
    ref = load_reference()
    check_facts(ref)
    out = {}
    with np.errstate(all="ignore"):
        for key, f in K.fixture_calls():
            out[key] = np.asarray(f(ref))
    for name in K.SIGNATURE_NAMES:
        out["sig_" + name] = np.array(str(inspect.signature(getattr(ref, name))))
    np.savez_compressed(OUT, **out)
    n_nan = sum(int(np.isnan(v).sum()) for k, v in out.items() if v.dtype == np.float64)
    n_inf = sum(int(np.isinf(v).sum()) for k, v in out.items() if v.dtype == np.float64)
    print("wrote %s: %d keys, %d bytes, %d NaN, %d inf" % (OUT, len(out), os.path.getsize(OUT), n_nan, n_inf))


if __name__ == "__main__":
    main()
