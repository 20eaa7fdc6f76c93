"""No GPU: the statement of the population distance summaries (tests/harness/distsum_ref.py) against the reference's own
outputs (tests/golden/distsum.npz), the reference's names and signatures, the ctypes mirrors against include/ia3.h, the
argument errors that come before any device call, the plotting-order helpers against the reference's outputs, and the
stand-alone check of csrc/ia3_distsum.h (tests/native/distsum_cpu.cpp), also under AddressSanitizer and UBSan."""
import functools
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import load_golden
from harness import distsum_cases as K
from harness import distsum_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def gold():
    return load_golden("distsum.npz")


@pytest.fixture(scope="module")
def D():
    from imageanalysis3_amd.structure_tools import distance
    return distance


@pytest.mark.parametrize("name", K.CASES)
def test_statement_equals_the_reference(gold, name):
    a, b, th = K.case(name)
    q = R.q_stack(a, b)
    nf, nc, prob = R.counts(q, th)
    for key, mine in (("median", R.median(q)), ("mean", R.mean(q)), ("prob", prob), ("nf", nf), ("nc", nc)):
        assert R.same_values(mine, gold["%s_%s" % (name, key)]), (name, key)


@pytest.mark.parametrize("function", ["median", "mean", "prob"])
def test_statement_of_the_dict_equals_the_reference(gold, function):
    name = {"median": "nanmedian", "mean": "nanmean", "prob": "contact"}[function]
    out = R.summary_dict(K.struct_cells(), K.struct_codebook(), name, K.STRUCT_TH)
    assert [K.key_name(k) for k in out] == list(gold["struct_keys"]) == [K.key_name(k) for k in K.STRUCT_KEYS]
    for k, m in out.items():
        assert R.same_values(m, gold["struct_%s_%s" % (function, K.key_name(k))]), k
    # the chromosome no cell has: NaN matrices sized from the codebook
    assert out["cis_X"].shape == (4, 4) and out[("2", "X")].shape == (7, 4) and np.isnan(out[("1", "X")]).all()


SIGNATURES = {
    "Chr2ZxysList_2_summaryDist_by_key": "(chr_2_zxys_list, _c1, _c2, codebook_df, function='nanmedian', axis=0, verbose=False)",
    "Chr2ZxysList_2_summaryDict": "(chr_2_zxys_list, total_codebook, function='nanmedian', axis=0, parallel=True, num_threads=12, "
                                  "verbose=False)",
    "sort_chr": "(_chr)",
    "Generate_PlotOrder": "(total_codebook, sel_codebook, sort_by_region=True)",
    "assemble_ChrDistDict_2_Matrix": "(dist_dict, total_codebook, sel_codebook=None, use_cis=True, use_trans=False, "
                                     "sort_by_region=True)",
    "generate_plot_chr_edges": "(sel_codebook, chr_2_plot_inds=None, sort_by_region=True)",
    "contact_prob": "(mat, contact_th=0.6, axis=0)",
}


def test_names_and_signatures_are_the_references(D):
    for name, sig in SIGNATURES.items():
        assert str(inspect.signature(getattr(D, name))) == sig, name
    assert D.default_num_threads == 12
    assert str(inspect.signature(D.population_distance_summary)) == \
        "(zxys_a, zxys_b=None, function='nanmedian', contact_th=None, return_counts=False)"


def test_ctypes_mirrors_match_the_header():
    from imageanalysis3_amd import _lib
    src = open(os.path.join(ROOT, "include", "ia3.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    found = re.findall(r"\b(?:int|void)\s+(ia3_dist_[a-z_]+)\s*\(", src)       # their prototypes: test_abi_cpu.py
    assert sorted(found) == sorted(e for e in _lib.EXPORTS if e.startswith("ia3_dist_")) and len(found) == 4
    enum = re.search(r"enum\s*\{\s*IA3_DIST_NANMEDIAN = (\d+), IA3_DIST_NANMEAN = (\d+), IA3_DIST_CONTACT = (\d+)\s*\}", src)
    assert [int(v) for v in enum.groups()] == [_lib.DIST_NANMEDIAN, _lib.DIST_NANMEAN, _lib.DIST_CONTACT]
    assert int(re.search(r"#define IA3_TUNE_DIST_TILE (\d+)", src).group(1)) == _lib.IA3_TUNE_DIST_TILE


def test_errors_come_before_any_device_call(D):
    """This test runs without a device: a call that reached the library would raise IA3Error instead."""
    cells, book = K.struct_cells(), K.struct_codebook()
    for bad in ("median", "nanmax", np.nanmedian, lambda m, axis: m, functools.partial(D.contact_prob, 0.5),
                functools.partial(D.contact_prob, th=0.5), functools.partial(np.nanmedian)):
        with pytest.raises(NotImplementedError, match="supported: function='nanmedian'"):
            D.Chr2ZxysList_2_summaryDist_by_key(cells, '1', '2', book, function=bad)
        with pytest.raises(NotImplementedError, match="supported"):
            D.Chr2ZxysList_2_summaryDict(cells, book, function=bad)
        with pytest.raises(NotImplementedError):
            D.population_distance_summary(np.zeros((2, 3, 3)), function=bad)
    for fn in ('nanmedian', D.contact_prob):
        with pytest.raises(NotImplementedError, match="axis=1"):
            D.Chr2ZxysList_2_summaryDist_by_key(cells, '1', '1', book, function=fn, axis=1)
        with pytest.raises(NotImplementedError, match="axis=1"):
            D.Chr2ZxysList_2_summaryDict(cells, book, function=fn, axis=1, parallel=False)
    with pytest.raises(NotImplementedError):
        D.contact_prob(np.zeros((2, 3)), axis=1)
    with pytest.raises(TypeError):
        D.Chr2ZxysList_2_summaryDist_by_key(cells, '1', '2', book, function=5)
    # matrices of unequal shape under one key
    ragged = [dict(c) for c in cells]
    ragged[0]['1'] = [np.zeros((6, 3))]
    with pytest.raises(ValueError, match="inhomogeneous"):
        D.Chr2ZxysList_2_summaryDist_by_key(ragged, '1', '2', book)
    with pytest.raises(ValueError, match="inhomogeneous"):
        D.Chr2ZxysList_2_summaryDict(ragged, book, parallel=False)
    with pytest.raises(ValueError):
        D.Chr2ZxysList_2_summaryDist_by_key([{'1': [np.zeros((5, 2))]}], '1', '1', book)
    with pytest.raises(ValueError):
        D.population_distance_summary(np.zeros((2, 3)))
    with pytest.raises(ValueError):
        D.population_distance_summary(np.zeros((2, 3, 3)), np.zeros((3, 3, 3)))


def test_no_cell_needs_no_device(D):
    """No copy of the pair anywhere: the NaN matrices come from the codebook alone."""
    book = K.struct_codebook()
    out = D.Chr2ZxysList_2_summaryDist_by_key(K.struct_cells(), 'X', 'X', book)
    assert list(out) == ["cis_X", "trans_X"] and all(m.shape == (4, 4) and np.isnan(m).all() for m in out.values())
    out = D.Chr2ZxysList_2_summaryDict([{}, {'1': None}], book, parallel=True, num_threads=3)
    assert [K.key_name(k) for k in out] == [K.key_name(k) for k in K.STRUCT_KEYS]
    assert out[('1', '2')].shape == (5, 7) and all(np.isnan(m).all() for m in out.values())


def test_qstar_statement():
    assert K.qstar(-0.5) == -1 and K.qstar(np.nan) == -1 and K.qstar(np.inf) == np.inf and K.qstar(0.0) == 0
    for th in (0.6, 0.5, 1.0, 3.0, 500.0):
        qs = K.qstar(th)
        assert np.sqrt(qs) <= th < np.sqrt(np.nextafter(qs, np.inf))
    assert np.sqrt(np.nextafter(K.qstar(0.6), -np.inf)) == 0.6       # two adjacent q share the root 0.6


def test_plotting_order_helpers_equal_the_reference(D, gold):
    pytest.importorskip("pandas")
    total, sel = K.plot_codebooks()
    assert [D.sort_chr(c) for c in ('1', '2', '10', 'X', 'Y')] == list(gold["plot_sort_keys"])
    with pytest.raises(UnboundLocalError):
        D.sort_chr('M')
    dist = {}
    for key in gold:
        if key.startswith("plot_dist_"):
            k = key[len("plot_dist_"):]
            dist[tuple(k.split("-")) if "-" in k else k] = gold[key]
    for by_region, tag in ((True, "region"), (False, "chr")):
        inds, orders = D.Generate_PlotOrder(total, sel, sort_by_region=by_region)
        assert list(inds) == list(orders) == list(gold["plot_%s_names" % tag])
        for c in inds:
            assert R.same_bits(np.asarray(inds[c]), gold["plot_%s_inds_%s" % (tag, c)])
            assert R.same_bits(np.asarray(orders[c]), gold["plot_%s_orders_%s" % (tag, c)])
        for cis, trans in ((True, False), (False, True)):
            m, edges, names = D.assemble_ChrDistDict_2_Matrix(dist, total, sel, use_cis=cis, use_trans=trans, sort_by_region=by_region)
            sub = "%s_%s" % (tag, "cis" if cis else "trans")
            assert R.same_values(m, gold["plot_%s_matrix" % sub]) and R.same_bits(edges, gold["plot_%s_edges" % sub])
            assert list(names) == list(gold["plot_%s_edgenames" % sub])
        edges, names = D.generate_plot_chr_edges(sel, None, sort_by_region=by_region)
        assert R.same_bits(edges, gold["plot_%s_own_edges" % tag]) and list(names) == list(gold["plot_%s_own_edgenames" % tag])


# ---- csrc/ia3_distsum.h on the host ------------------------------------------------------------------------------------------

SRC = os.path.join(HERE, "native", "distsum_cpu.cpp")
HDR = os.path.join(ROOT, "imageanalysis3_amd", "csrc", "ia3_distsum.h")
EXE = os.path.join(HERE, "native", "distsum_cpu")


def _build(exe, extra=()):
    if not os.path.isfile(exe) or os.path.getmtime(exe) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off"] + list(extra) + ["-o", exe, SRC])
    return exe


def _run(exe):
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-2000:]
    m = re.search(r"thresholds (\d+), predicates (\d+), selects (\d+), mismatches (\d+)", p.stdout)
    assert m, p.stdout
    sums = {int(n): bits for n, bits in re.findall(r"pairwise (\d+) ([0-9a-f]{16})", p.stdout)}
    return [int(v) for v in m.groups()], sums


def _check(result):
    (thresholds, predicates, selects, bad), sums = result
    assert bad == 0 and thresholds > 200000 and predicates > 10 * thresholds and selects > 20000
    # NumPy's pairwise order over a contiguous axis, what np.nanmean takes for a stack of 1 x 1 matrices
    assert sorted(sums) == [1, 7, 8, 9, 128, 129, 136, 641, 5000, 100003]
    for n, bits in sums.items():
        i = np.arange(n, dtype=np.uint64)
        v = (i * np.uint64(2654435761) % np.uint64(4294967296)).astype(np.float64) / 4294967296.0 * 3000.0
        assert np.float64(np.add.reduce(v)).tobytes() == np.uint64(int(bits, 16)).tobytes(), n


def test_qstar_select_and_pairwise_on_the_host():
    _check(_run(_build(EXE)))


def test_qstar_select_and_pairwise_under_sanitizers():
    """the same stand-alone program with AddressSanitizer and UBSan (a host program of its own: nothing is preloaded)"""
    _check(_run(_build(EXE + "_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])))
