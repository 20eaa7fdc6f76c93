"""GPU: the population distance summaries on the device (csrc/distsum.hip) against the statement
tests/harness/distsum_ref.py and against the reference's own outputs (tests/golden/distsum.npz), through the C entry
(``_lib.DistancePopulation``, ``population_distance_summary``) and through the reference-named functions.

Every comparison is bit for bit, a NaN for a NaN: no output depends on anything but IEEE float64 operations and counts.
The median kernel has one path with three tiles (2 x 2, 4 x 4 and 8 x 8 entries per workgroup, IA3_TUNE_DIST_TILE): every
case runs through all of them.  Every device call is made twice and must return the same bytes."""
import functools
import warnings

import numpy as np
import pytest

from conftest import load_golden
from harness import distsum_cases as K
from harness import distsum_ref as R

pytestmark = pytest.mark.gpu

FUNCTIONS = (("median", "nanmedian"), ("mean", "nanmean"), ("prob", "contact"))


@pytest.fixture(scope="module")
def L():
    from imageanalysis3_amd import _lib
    _lib.check(_lib.lib().ia3_init(0))
    yield _lib
    _lib.check(_lib.lib().ia3_set_tuning(_lib.IA3_TUNE_DIST_TILE, 0))


@pytest.fixture(scope="module")
def D(L):
    from imageanalysis3_amd.structure_tools import distance
    return distance


@pytest.fixture(scope="module")
def gold():
    return load_golden("distsum.npz")


_statements = {}


def statement(name):
    """The statement's outputs of a flat case, made once."""
    if name not in _statements:
        a, b, th = K.case(name)
        q = R.q_stack(a, b)
        nf, nc, prob = R.counts(q, th)
        _statements[name] = dict(median=R.median(q), mean=R.mean(q), prob=prob, nf=nf, nc=nc)
    return _statements[name]


def function_of(D, fname, th):
    return functools.partial(D.contact_prob, contact_th=th) if fname == "contact" else fname


def twice(call):
    """The call's outputs, made twice with identical bytes."""
    one, two = call(), call()
    one = one if isinstance(one, tuple) else (one,)
    two = two if isinstance(two, tuple) else (two,)
    assert len(one) == len(two) and all(x.tobytes() == y.tobytes() for x, y in zip(one, two))
    return one if len(one) > 1 else one[0]


@pytest.mark.parametrize("tile", [2, 4, 8])
@pytest.mark.parametrize("name", K.CASES)
def test_c_entry_equals_statement_and_reference(L, D, gold, name, tile):
    a, b, th = K.case(name)
    want = statement(name)
    L.check(L.lib().ia3_set_tuning(L.IA3_TUNE_DIST_TILE, tile))
    for key, fname in FUNCTIONS:
        out, nf, nc = twice(lambda: D.population_distance_summary(a, b, function=function_of(D, fname, th), contact_th=th,
                                                                  return_counts=True))
        assert out.dtype == np.float64 and nf.dtype == nc.dtype == np.int32
        for got, k in ((out, key), (nf, "nf"), (nc, "nc")):
            assert R.same_values(got, want[k]), (name, fname, k)
            assert R.same_values(got, gold["%s_%s" % (name, k)]), (name, fname, k)
        plain = D.population_distance_summary(a, b, function=function_of(D, fname, th))
        assert plain.tobytes() == out.tobytes()


@pytest.mark.parametrize("name", K.CASES)
def test_reference_named_function_on_flat_cases(L, D, gold, name):
    a, b, th = K.case(name)
    cells, (c1, c2) = K.as_cells(a, b)
    book = {'chr': np.array(['1'] * a.shape[1] + ['2'] * (a.shape[1] if b is None else b.shape[1]))}
    key = "cis_1" if b is None else ('1', '2')
    L.check(L.lib().ia3_set_tuning(L.IA3_TUNE_DIST_TILE, 0))
    for k, fname in FUNCTIONS:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            out = D.Chr2ZxysList_2_summaryDist_by_key(cells, c1, c2, book, function=function_of(D, fname, th))
        assert list(out) == (["cis_1", "trans_1"] if b is None else [key])
        assert R.same_values(out[key], gold["%s_%s" % (name, k)]) and R.same_values(out[key], statement(name)[k]), (name, k)
        if b is None:      # one copy per cell: no trans matrix, NaNs sized from the codebook
            assert out["trans_1"].shape == out[key].shape and np.isnan(out["trans_1"]).all()
        if np.isnan(out[key]).any():
            assert any(issubclass(x.category, RuntimeWarning) for x in w), (name, k)
        else:
            assert not any(issubclass(x.category, RuntimeWarning) for x in w)
    # contact_prob of the stack itself: `<= th` on the given values
    with np.errstate(invalid="ignore"):
        stack = np.sqrt(R.q_stack(a, b))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = twice(lambda: D.contact_prob(list(stack), contact_th=th))
        assert R.same_values(got, gold[name + "_stackprob"])
        with np.errstate(invalid="ignore", divide="ignore"):
            assert R.same_values(got, np.sum(stack <= th, axis=0) / np.sum(np.isfinite(stack), axis=0))


@pytest.mark.parametrize("tile", [2, 4, 8])
def test_summary_dict_equals_reference_and_statement(L, D, gold, tile):
    cells, book = K.struct_cells(), K.struct_codebook()
    L.check(L.lib().ia3_set_tuning(L.IA3_TUNE_DIST_TILE, tile))
    for k, fname in FUNCTIONS:
        fn = function_of(D, fname, K.STRUCT_TH)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out = D.Chr2ZxysList_2_summaryDict(cells, book, function=fn, parallel=True, num_threads=4)
            again = D.Chr2ZxysList_2_summaryDict(cells, book, function=fn, parallel=False)
            one = D.Chr2ZxysList_2_summaryDist_by_key(cells, '1', '2', book, function=fn)
        want = R.summary_dict(cells, book, fname, K.STRUCT_TH)
        assert list(out) == list(want) == list(again) and [K.key_name(x) for x in out] == list(gold["struct_keys"])
        assert all(isinstance(x, str) or isinstance(x, tuple) for x in out)
        for key, m in out.items():
            assert m.tobytes() == again[key].tobytes()
            assert R.same_values(m, want[key]) and R.same_values(m, gold["struct_%s_%s" % (k, K.key_name(key))]), (fname, key)
        assert list(one) == [('1', '2')] and one[('1', '2')].tobytes() == out[('1', '2')].tobytes()


def test_default_tile_choice_on_a_wide_map(L, D):
    """190 x 185: more 4 x 4 tiles than two per compute unit, so the default takes the 4 x 4 tile (the small cases take 2 x 2);
    every forced tile and the default give the statement's bits (N = 3: entries with 0 to 3 values)."""
    a, b = K._random(9, 3, 190, 185)
    q = R.q_stack(a, b)
    nf, nc, prob = R.counts(q, K.TH_DEFAULT)
    outs = []
    for tile in (0, 2, 4, 8):
        L.check(L.lib().ia3_set_tuning(L.IA3_TUNE_DIST_TILE, tile))
        outs.append(twice(lambda: D.population_distance_summary(a, b)))
    L.check(L.lib().ia3_set_tuning(L.IA3_TUNE_DIST_TILE, 0))
    assert all(R.same_values(o, R.median(q)) for o in outs)
    mean, got_nf, got_nc = D.population_distance_summary(a, b, function='nanmean', contact_th=K.TH_DEFAULT, return_counts=True)
    assert R.same_values(mean, R.mean(q)) and R.same_bits(got_nf, nf) and R.same_bits(got_nc, nc)
    cis = D.population_distance_summary(a)
    assert R.same_values(cis, R.median(R.q_stack(a))) and (np.diag(cis) == 0).all()


def test_threshold_edges(L, D):
    a, b, _ = K.case("infinite")
    q = R.q_stack(a, b)
    for th in (np.inf, -1.0, np.nan, 0.0):
        prob, nf, nc = D.population_distance_summary(a, b, function=D.contact_prob, contact_th=th, return_counts=True)
        want_nf, want_nc, want = R.counts(q, th)
        assert R.same_bits(nf, want_nf) and R.same_bits(nc, want_nc) and R.same_values(prob, want)
    with np.errstate(invalid="ignore"):
        # +inf: every value that is not NaN is a contact, inf included; negative or NaN: none
        assert R.same_bits(R.counts(q, np.inf)[1], (~np.isnan(q)).sum(axis=0).astype(np.int32))
    assert (R.counts(q, -1.0)[1] == 0).all() and (R.counts(q, np.nan)[1] == 0).all()


def test_library_argument_errors(L):
    import ctypes as C
    rs = np.random.RandomState(0)
    with L.DistancePopulation.upload([rs.rand(5, 3), rs.rand(5, 3), rs.rand(7, 3)]) as pop:
        out = np.zeros((5, 7))
        pa, pb = np.array([0, 1], dtype=np.int32), np.array([2, 2], dtype=np.int32)

        def rc(a, b, n, Ra, Rb, same=0, fn=L.DIST_NANMEDIAN):
            return L.lib().ia3_dist_summary_dev(pop._h, L._iptr(a), L._iptr(b), n, Ra, Rb, same, fn, C.c_double(1.0), L.dptr(out),
                                                None, None)

        assert rc(pa, pb, 2, 5, 7) == L.IA3_OK
        assert rc(pa, pb, 0, 5, 7) == L.IA3_EINVAL                                           # N < 1
        assert rc(np.array([0, 3], dtype=np.int32), pb, 2, 5, 7) == L.IA3_EINVAL             # copy index out of range
        assert rc(np.array([0, -1], dtype=np.int32), pb, 2, 5, 7) == L.IA3_EINVAL
        assert rc(pa, pb, 2, 7, 5) == L.IA3_EINVAL                                           # rows other than Ra / Rb
        assert rc(pa, np.array([2, 1], dtype=np.int32), 2, 5, 7) == L.IA3_EINVAL
        assert rc(pa, pa[::-1].copy(), 2, 5, 5, same=1) == L.IA3_EINVAL                      # same, but another copy
        assert rc(pa, pb, 2, 5, 7, fn=7) == L.IA3_EINVAL
        with pytest.raises(ValueError):
            pop.summary([0, 1], [2, 3])
        with pytest.raises(ValueError):
            pop.summary([0, 2], [2, 2])
        with pytest.raises(ValueError):
            pop.summary([], [])
