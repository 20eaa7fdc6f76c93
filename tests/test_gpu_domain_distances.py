"""GPU: the domain distances on the device (csrc/domain.hip) against the reference's own outputs
(tests/golden/domain_distances.npz) through the flat forms on a resident population and the reference-named functions.

Every finite value, infinity and zero equals the reference's in every bit; a NaN stands where the reference has a NaN (its
sign and payload are not compared: the host's 0.0 / 0.0 is the negative quiet NaN, the device's is not).  Every call runs
twice and every copy alone and in the batch, and the bytes are compared."""
import numpy as np
import pytest

from conftest import load_golden
from harness import domain_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from imageanalysis3_amd import _lib
    _lib.check(_lib.lib().ia3_init(0))
    return _lib


@pytest.fixture(scope="module")
def D(L):
    from imageanalysis3_amd.domain_tools import distance
    return distance


@pytest.fixture(scope="module")
def gold():
    return load_golden("domain_distances.npz")


def _twice(f):
    a, b = f(), f()
    assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
    return a


def _sources(L, norm=None):
    """(name, batch population, one population per copy, the copies) of the domain cases."""
    out = []
    for name, pop in K.domain_populations().items():
        out.append((name, L.DomainPopulation.upload(pop, norm), [L.DomainPopulation.upload(z, norm) for z in pop], list(pop)))
    m = K.domain_map()
    out.append(("map", L.DomainPopulation.upload_matrix(m, norm), [L.DomainPopulation.upload_matrix(m, norm)], [m]))
    return out


def test_windows_equal_the_reference(L, D, gold):
    pops = [(name, L.DomainPopulation.upload(z), [L.DomainPopulation.upload(c) for c in z]) for name, z in K.window_populations().items()]
    pops.append(("map", L.DomainPopulation.upload_matrix(K.window_map()), [L.DomainPopulation.upload_matrix(K.window_map())]))
    for name, pop, alone in pops:
        for metric in K.WINDOW_METRICS:
            got = _twice(lambda: D.population_sliding_window_dists(pop, K.WDS, metric))
            want = gold["win_%s_%s" % (name, metric)]
            assert got.shape == want.shape and got.dtype == np.float64
            assert K.same(got, want), (name, metric, np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))[:5])
            for n, one in enumerate(alone):
                assert one.slide(K.WDS, metric).tobytes() == got[n:n + 1].tobytes(), (name, metric, n)
            # a call with one window size is the row of the call with all
            assert pop.slide([K.WDS[3]], metric).tobytes() == np.ascontiguousarray(got[:, 3:4]).tobytes()
    # the reference's name, on a map
    m = K.window_map()
    for wd, metric in ((5, 'median'), (16, 'ks'), (9, 'mean')):
        row = D._sliding_window_dist(m, wd, metric)
        assert row.shape == (K.R_WIN,) and K.same(row, gold["win_map_%s" % metric][0, K.WDS.index(wd)])
    assert D._sliding_window_dist(m, 5).tobytes() == D._sliding_window_dist(m, 5, 'median').tobytes()
    for _, pop, alone in pops:
        pop.free()
        [a.free() for a in alone]


def test_domain_pdists_equal_the_reference(L, D, gold):
    for nm, norm in (("raw", None), ("norm", K.normalization())):
        for name, pop, alone, copies in _sources(L, norm):
            if name == "lattice" and nm == "norm":
                continue
            for metric in K.DIST_METRICS:
                for allow in (False, True):
                    got = _twice(lambda: np.array(D.population_domain_pdists(pop, [K.STARTS] * pop.N, metric, allow), dtype=np.float64))
                    want = gold["pd_%s_%s_%d_%s" % (name, metric, allow, nm)]
                    assert K.same(got, want), (name, metric, allow, nm, got, want)
                    for n, one in enumerate(alone):
                        a = np.array(D.population_domain_pdists(one, [K.STARTS], metric, allow), dtype=np.float64)
                        assert a.tobytes() == got[n:n + 1].tobytes(), (name, metric, allow, nm, n)
            # the reference's name against the flat form
            named = D.domain_pdists(copies[-1], K.STARTS, normalization_mat=norm)
            flat = D.population_domain_pdists(pop, [K.STARTS] * pop.N)[-1]
            # np.array of the reference's results is an integer array where every pair gave Python's integer 0
            assert flat.dtype == np.float64 and named.dtype in (np.float64, np.array([0]).dtype)
            assert named.dtype == np.float64 or not (flat.any() or np.isnan(flat).any())
            assert named.astype(np.float64).tobytes() == flat.tobytes()
            assert K.same(named, gold["pd_%s_median_0_%s" % (name, nm)][-1])


def test_neighboring_dists_equal_the_reference(L, D, gold):
    for nm, norm in (("raw", None), ("norm", K.normalization())):
        for name, pop, alone, copies in _sources(L, norm):
            for use_local, mds in K.NEIGHBOR_OPTIONS:
                got = _twice(lambda: np.array(D.population_domain_neighboring_dists(pop, [K.STARTS] * pop.N, use_local=use_local,
                                                                                    min_dom_sz=mds), dtype=np.float64))
                want = gold["nb_%s_%d_%d_%s" % (name, use_local, mds, nm)]
                assert K.same(got, want), (name, use_local, mds, nm, got, want)
                for n, one in enumerate(alone):
                    a = np.array(D.population_domain_neighboring_dists(one, [K.STARTS], use_local=use_local, min_dom_sz=mds), dtype=np.float64)
                    assert a.tobytes() == got[n:n + 1].tobytes()
                named = D.domain_neighboring_dists(copies[0], K.STARTS, use_local=use_local, min_dom_sz=mds, normalization_mat=norm)
                assert K.same(named, want[0])


def test_single_calls_return_the_references_types(L, D, gold):
    for name, pop, alone, copies in _sources(L):
        res = [D.domain_distance(copies[-1], b1, b2, _metric=metric, _allow_minus_distance=allow)
               for b1, b2 in K.SINGLE_CALLS for metric in K.DIST_METRICS for allow in (True, False)]
        values, zero = K.as_float(res)
        assert np.array_equal(zero, gold["dd_%s_intzero" % name]) and K.same(values, gold["dd_%s_values" % name]), name
        assert all(type(r) is (int if z else np.float64) for r, z in zip(res, zero))
        # the entries of one call do not depend on each other: the same entries in one call
        quads = [(pop.N - 1,) + tuple(b1) + tuple(b2) for b1, b2 in K.SINGLE_CALLS]
        v, z = _twice(lambda: np.concatenate(pop.distances(quads, 'median', True))), None
        assert K.same(v[:len(quads)], values[0::6]) and np.array_equal(v[len(quads):] != 0, zero[0::6])


def test_contact_frequencies_equal_the_reference(L, D, gold):
    for name, pop, alone, copies in _sources(L):
        ths = K.lattice_thresholds() if name == "lattice" else [400, -1.0]
        for k, th in enumerate(ths):
            for sn, starts in (("a", K.STARTS), ("b", K.CONTACT_STARTS)):
                got = _twice(lambda: np.array(D.population_domain_contact_freq(pop, [starts] * pop.N, th)))
                want = gold["cf_%s_%d_%s" % (name, k, sn)]
                assert K.same(got, want), (name, th, sn)
                for n, one in enumerate(alone):
                    assert np.array(D.population_domain_contact_freq(one, [starts], th)).tobytes() == got[n:n + 1].tobytes()
                named = D._domain_contact_freq(copies[0], starts, th)
                assert named.tobytes() == got[0].tobytes()
        if name == "lattice":
            assert (gold["cf_lattice_1_a"] != gold["cf_lattice_0_a"]).any() and not gold["cf_lattice_3_a"].any()
