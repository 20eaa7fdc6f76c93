"""Fixtures of the population distance summaries: tests/golden/distsum.npz.

Runs the reference's own ``structure_tools/distance.py`` (``Chr2ZxysList_2_summaryDist_by_key``,
``Chr2ZxysList_2_summaryDict`` with ``parallel=False``, ``contact_prob`` and the plotting-order helpers) on the cases of
tests/harness/distsum_cases.py.  The module is loaded by file as oracle/ref_loader.py loads the others, with a stand-in for
``tqdm`` where it is not installed.  Only outputs are stored: per flat case the nanmedian, the nanmean, the contact
probability and the two counts the reference's stack gives; per key of the codebook case the three summaries; the outputs
of the plotting-order helpers.  Needs the reference tree (IA3_REFERENCE), pandas and SciPy; nothing here runs on the GPU.

    python scripts/make_distsum_golden.py

The script asserts what the tests rely on: that tests/harness/distsum_ref.py reproduces every stored array byte for byte
(a NaN for a NaN), and the facts about SciPy's and NumPy's arithmetic that csrc/distsum.hip is built on.
"""
import functools
import importlib.util
import os
import sys
import types
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

OUT = os.path.join(ROOT, "tests", "golden")


def load_module():
    import ref_loader
    if "tqdm" not in sys.modules:
        try:
            import tqdm  # noqa: F401
        except ImportError:
            sys.modules["tqdm"] = types.ModuleType("tqdm")
            sys.modules["tqdm"].tqdm = lambda it, *a, **k: it
    spec = importlib.util.spec_from_file_location("IA3_structure_distance",
                                                  os.path.join(ref_loader.REF, "structure_tools", "distance.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def facts(K, R):
    """The CPU facts of the arithmetic (NumPy / SciPy of this host)."""
    from scipy.spatial.distance import cdist, pdist, squareform
    rs = np.random.RandomState(0)
    a, b = rs.normal(0, 400, (40, 3)), rs.normal(0, 400, (30, 3))
    a[3] = np.nan
    assert R.same_values(cdist(a, b), np.sqrt(R.q_stack(a[None], b[None])[0]))
    sq = squareform(pdist(a))
    assert R.same_values(sq, np.sqrt(R.q_stack(a[None])[0])) and (np.diag(sq) == 0).all() and sq[3, 3] == 0 and np.isnan(sq[3, 4])
    # nanmedian on both of NumPy's paths, with NaNs, whole-NaN entries and inf
    for N in (1, 2, 5, 64, 599, 600, 601, 700):
        v = rs.uniform(0, 3000, (N, 4, 5))
        v[rs.rand(N, 4, 5) < 0.3] = np.nan
        v[rs.rand(N, 4, 5) < 0.05] = np.inf
        v[:, 0, 0] = np.nan
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            got = np.nanmedian(list(v), axis=0)
        assert any(issubclass(x.category, RuntimeWarning) and "All-NaN slice" in str(x.message) for x in w), N
        assert R.same_values(got, R.median(v * v)), N        # v = sqrt(v * v) for these magnitudes? checked next
        assert (np.sqrt(v * v)[~np.isnan(v)] == v[~np.isnan(v)]).all()
    # nanmean: sequential over n, pairwise for a stack of 1 x 1 matrices
    for N, shape in ((1000, (3, 4)), (1000, (1, 2)), (1000, (1, 1)), (129, (1, 1)), (9, (1, 1))):
        v = rs.uniform(0, 3000, (N,) + shape)
        v[rs.rand(*v.shape) < 0.3] = np.nan
        assert R.same_values(np.nanmean(list(v), axis=0), R.mean(v * v)), (N, shape)
    seq = 0.0
    v = rs.uniform(0, 3000, 1000)
    for x in v:
        seq += x
    assert np.nanmean(list(v.reshape(-1, 1, 1)), axis=0)[0, 0] != seq / 1000       # the degenerate shape is NOT sequential
    # q* is at most one step from th * th, and adjacent q share a root
    ths = np.concatenate([rs.uniform(0, 2000, 20000), [0.6, 0.5, 1.0, 3.0, 500.0]])
    for th in ths:
        qs = K.qstar(th)
        assert np.sqrt(qs) <= th < np.sqrt(np.nextafter(qs, np.inf))
        assert qs in (th * th, np.nextafter(th * th, np.inf), np.nextafter(th * th, -np.inf)), th
    q06 = K.qstar(0.6)
    assert np.sqrt(np.nextafter(q06, -np.inf)) == np.sqrt(q06) == 0.6
    assert K.qstar(-1.0) == -1 and K.qstar(np.nan) == -1 and K.qstar(np.inf) == np.inf


def main():
    import pandas as pd
    from harness import distsum_cases as K
    from harness import distsum_ref as R
    ref = load_module()
    facts(K, R)
    d = {}
    warnings.simplefilter("ignore")
    for name in K.CASES:
        a, b, th = K.case(name)
        cells, (c1, c2) = K.as_cells(a, b)
        book = pd.DataFrame({'chr': ['1'] * a.shape[1] + ['2'] * (a.shape[1] if b is None else b.shape[1])})
        key = "cis_1" if b is None else ('1', '2')
        q = R.q_stack(a, b)

        def run(function):
            out = ref.Chr2ZxysList_2_summaryDist_by_key(cells, c1, c2, book, function=function)
            assert list(out) == (["cis_1", "trans_1"] if b is None else [key]), list(out)
            return out[key]

        got = {"median": run('nanmedian'), "mean": run('nanmean'),
               "prob": run(functools.partial(ref.contact_prob, contact_th=th)),
               "nf": run(lambda m, axis: np.sum(np.isfinite(m), axis=axis)).astype(np.int32),
               "nc": run(lambda m, axis: np.sum(np.array(m) <= th, axis=axis)).astype(np.int32)}
        nf, nc, prob = R.counts(q, th)
        mine = {"median": R.median(q), "mean": R.mean(q), "prob": prob, "nf": nf, "nc": nc}
        for k in got:
            assert R.same_values(got[k], mine[k]), (name, k)
            d["%s_%s" % (name, k)] = got[k]
        # the stack contact_prob of the given values
        stack = np.sqrt(q)
        d[name + "_stackprob"] = ref.contact_prob(list(stack), contact_th=th)
        c = (~np.isnan(q)).sum(axis=0)
        print(name, q.shape, "counts", sorted(set(c.ravel().tolist()))[:6], "nan entries", int(np.isnan(got["median"]).sum()))
        if name == "shared_roots":
            s = np.sort(q, axis=0)
            shared = ((s[1:] != s[:-1]) & (np.sqrt(s[1:]) == np.sqrt(s[:-1]))).sum(axis=0)
            assert (shared > 0).all(), shared
            print("   distinct neighbours with one root per entry:", int(shared.min()), "..", int(shared.max()))
        if name == "ties":
            s = np.sort(q, axis=0)
            lo, hi = np.take_along_axis(s, (c[None] - 1) // 2, 0)[0], np.take_along_axis(s, c[None] // 2, 0)[0]
            assert ((lo == hi) & (c % 2 == 0)).sum() > 10
        if name.startswith("contact"):
            qs = K.qstar(th)
            assert (q[:, 0, 0] == np.nextafter(qs, -np.inf)).all() and (q[:, 1, 0] == qs).all() and (q[:, 2, 0] == np.nextafter(qs, np.inf)).all()
            assert (got["nc"][:3, 0] == [len(q), len(q), 0]).all()
            if th == 5.0:
                assert (np.sqrt(q[:, 3, 0]) == 5.0).all() and got["nc"][3, 0] == len(q)
    # the codebook structure
    cells, book = K.struct_cells(), K.struct_codebook()
    frame = pd.DataFrame(book)
    for function, fname in (('nanmedian', "median"), ('nanmean', "mean"),
                            (functools.partial(ref.contact_prob, contact_th=K.STRUCT_TH), "prob")):
        out = ref.Chr2ZxysList_2_summaryDict(cells, frame, function=function, parallel=False)
        assert [K.key_name(k) for k in out] == [K.key_name(k) for k in K.STRUCT_KEYS], list(out)
        mine = R.summary_dict(cells, book, "nanmedian" if fname == "median" else "nanmean" if fname == "mean" else "contact", K.STRUCT_TH)
        assert list(mine) == list(out)
        for k, m in out.items():
            assert R.same_values(m, mine[k]), (fname, k)
            d["struct_%s_%s" % (fname, K.key_name(k))] = m
        one = ref.Chr2ZxysList_2_summaryDist_by_key(cells, '1', '2', frame, function=function)
        assert list(one) == [('1', '2')] and R.same_values(one[('1', '2')], out[('1', '2')])
    d["struct_keys"] = np.array([K.key_name(k) for k in K.STRUCT_KEYS])
    # the plotting-order helpers
    total, sel = K.plot_codebooks()
    d["plot_sort_keys"] = np.array([ref.sort_chr(c) for c in ('1', '2', '10', 'X', 'Y')], dtype=np.int64)
    rs = np.random.RandomState(5)
    sizes = {c: int((total['chr'] == c).sum()) for c in np.unique(total['chr'])}
    dist = {}
    for c in sizes:
        dist["cis_%s" % c] = rs.rand(sizes[c], sizes[c])
        dist["trans_%s" % c] = rs.rand(sizes[c], sizes[c])
    dist[('1', '2')] = rs.rand(sizes['1'], sizes['2'])
    dist[('X', '1')] = rs.rand(sizes['X'], sizes['1'])
    dist[('10', 'X')] = rs.rand(sizes['10'], sizes['X'])
    for c in sizes:
        d["plot_dist_cis_%s" % c], d["plot_dist_trans_%s" % c] = dist["cis_%s" % c], dist["trans_%s" % c]
    d["plot_dist_1-2"], d["plot_dist_X-1"], d["plot_dist_10-X"] = dist[('1', '2')], dist[('X', '1')], dist[('10', 'X')]
    for by_region in (True, False):
        tag = "region" if by_region else "chr"
        inds, orders = ref.Generate_PlotOrder(total, sel, sort_by_region=by_region)
        d["plot_%s_names" % tag] = np.array(list(inds))
        for c in inds:
            d["plot_%s_inds_%s" % (tag, c)], d["plot_%s_orders_%s" % (tag, c)] = np.asarray(inds[c]), np.asarray(orders[c])
        for cis, trans in ((True, False), (False, True)):
            m, edges, names = ref.assemble_ChrDistDict_2_Matrix(dist, total, sel, use_cis=cis, use_trans=trans, sort_by_region=by_region)
            sub = "%s_%s" % (tag, "cis" if cis else "trans")
            d["plot_%s_matrix" % sub], d["plot_%s_edges" % sub], d["plot_%s_edgenames" % sub] = m, edges, np.array(names)
        edges, names = ref.generate_plot_chr_edges(sel, None, sort_by_region=by_region)
        d["plot_%s_own_edges" % tag], d["plot_%s_own_edgenames" % tag] = edges, np.array(names)
    d["source"] = np.array("reference")
    path = os.path.join(OUT, "distsum.npz")
    np.savez_compressed(path, **d)
    print("arrays", len(d), "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
