"""No GPU: the reference's names and signatures of domain_tools/distance.py, the argument errors that come before any
device call, the NumPy statement of the arithmetic (tests/harness/domain_cases.py) against the fixture
(tests/golden/domain_distances.npz, the reference's own outputs) bit for bit, the ctypes mirrors against include/ia3.h, and
the stand-alone check of csrc/ia3_domain.h (tests/native/domain_cpu.cpp) against values of the fixture, also under
AddressSanitizer and UBSan."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import load_golden
from harness import domain_cases as K

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def gold():
    return load_golden("domain_distances.npz")


@pytest.fixture(scope="module")
def D():
    from imageanalysis3_amd.domain_tools import distance
    return distance


@pytest.fixture()
def no_device(monkeypatch):
    """Any call into the library fails the test: the errors below come before it."""
    from imageanalysis3_amd import _lib

    def refuse():
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "lib", refuse)
    return _lib


def test_signatures_are_the_references(D, gold):
    for name in K.SIGNATURE_NAMES:
        assert str(inspect.signature(getattr(D, name))) == str(gold["sig_" + name]), name


def test_fixture_holds_what_the_cases_need(gold):
    assert os.path.getsize(os.path.join(HERE, "golden", "domain_distances.npz")) < 300000
    keys = [k for k, _ in K.fixture_calls()]
    assert sorted(keys + ["sig_" + n for n in K.SIGNATURE_NAMES]) == sorted(gold)
    lat = gold["win_lattice_median"]
    assert lat.shape == (K.N_WIN, len(K.WDS), K.R_WIN)
    assert np.isnan(lat).any() and np.isinf(lat).any()          # v_inter + v_intra == 0
    assert gold["dd_walk_intzero"].any() and not gold["dd_walk_intzero"].all()
    assert (gold["win_short_median"][:, K.WDS.index(9)] == 0).all() and not gold["win_one_mean"].any()


def test_numpy_statement_equals_the_fixture(gold):
    for key, f in K.fixture_calls():
        got = np.asarray(f(K.numpy_namespace))
        if got.dtype == bool:
            assert np.array_equal(got, gold[key]), key
        else:
            assert K.same(got, gold[key]), key


def test_argument_errors_come_before_the_device(D, no_device):
    L = no_device
    z = np.zeros((10, 3))
    m = np.zeros((10, 10))
    with pytest.raises(ValueError):
        D._sliding_window_dist(z, 3)                       # the map only
    with pytest.raises(ValueError):
        D._sliding_window_dist(m, 3, 'other')
    with pytest.raises(ValueError):
        D._sliding_window_dist(m, 0)
    with pytest.raises(NotImplementedError):
        D._sliding_window_dist(m, L.IA3_DOMAIN_MAX_WINDOW + 1)
    for bad in (np.zeros(10), np.zeros((10, 4)), np.zeros((2, 3, 3))):
        with pytest.raises(ValueError):
            D.domain_distance(bad, (0, 2), (2, 4))
        with pytest.raises(ValueError):
            D.domain_pdists(bad, [0, 5])
        with pytest.raises(ValueError):
            D.domain_neighboring_dists(bad, [0, 5])
    with pytest.raises(ValueError):
        D.domain_distance(z, (0, 2), (2, 4), _metric='other')
    for metric in ('mean', 'ks', 'KS'):
        with pytest.raises(NotImplementedError):
            D.domain_distance(z, (0, 2), (2, 4), _metric=metric)
        with pytest.raises(NotImplementedError):
            D.domain_pdists(z, [0, 5], metric=metric)
    with pytest.raises(ValueError):
        D.domain_distance(z, (-1, 2), (2, 4))
    with pytest.raises(ValueError):
        D.domain_pdists(z, [0, 5], normalization_mat=np.zeros((9, 9)))
    with pytest.raises(ValueError):
        D.domain_neighboring_dists(z, [0, 5], normalization_mat=np.zeros((9, 10)))
    with pytest.raises(IndexError):
        D.domain_pdists(z, [])
    with pytest.raises(ValueError):
        D._domain_contact_freq(np.zeros((10, 4)), [0, 5])
    with pytest.raises(ValueError):
        D._domain_contact_freq(z, [0, 12])
    # the normalisation map: the words of squareform, which the reference runs on the diagonal blocks
    sym = np.ones((10, 10)) - np.eye(10)
    asym = sym.copy()
    asym[2, 3] = 2.
    with pytest.raises(ValueError, match="must be symmetric"):
        L.DomainPopulation.upload(z, asym)
    with pytest.raises(ValueError, match="diagonal must be zero"):
        L.DomainPopulation.upload(z, sym + np.eye(10))
    with pytest.raises(ValueError):
        L.DomainPopulation.upload(np.zeros((2, 10, 4)))
    with pytest.raises(ValueError):
        L.DomainPopulation.upload_matrix(np.zeros((10, 9)))
    with pytest.raises(NotImplementedError):
        L.DomainPopulation.upload(np.zeros((1, L.IA3_DOMAIN_MAX_R + 1, 3)))
    pop = L.DomainPopulation(None, 2, 10, False, False)
    with pytest.raises(ValueError):
        pop.slide([])
    with pytest.raises(ValueError):
        pop.slide(list(range(1, L.IA3_DOMAIN_MAX_WINDOWS + 2)))
    with pytest.raises(NotImplementedError):
        pop.slide([3, 17])
    with pytest.raises(ValueError):
        pop.slide([3], 'other')
    with pytest.raises(ValueError):
        pop.slide([3], normalize=True)                     # no map
    for quads in ([(2, 0, 2, 2, 4)], [(0, 0, 11, 2, 4)], [(0, 3, 2, 2, 4)], [(0, 0, 2, 2)], []):
        with pytest.raises(ValueError):
            pop.distances(quads)
        with pytest.raises(ValueError):
            pop.contacts(quads)
    with pytest.raises(ValueError):
        pop.distances([(0, 0, 2, 2, 4)], 'mean')
    with pytest.raises(ValueError):
        D.population_domain_pdists(pop, [[0, 5]])          # one list per copy
    with pytest.raises(NotImplementedError):
        D.population_domain_pdists(pop, [[0, 5], [0, 5]], metric='ks')


def test_what_is_not_built_says_so(D):
    z = np.zeros((10, 3))
    for call in (lambda: D.domain_stat(z, (0, 2), (2, 4)), lambda: D.domain_neighboring_stats(z, [0, 5]),
                 lambda: D.domain_correlation_pdists(z, [0, 5]), lambda: D._local_distances(z), lambda: D._neighboring_distance(z)):
        with pytest.raises(NotImplementedError) as e:
            call()
        assert "not built" in str(e.value) and len(str(e.value)) > 40
    for name in ("calling", "interaction", "manual"):
        with pytest.raises(ImportError):
            __import__("imageanalysis3_amd.domain_tools." + name)


def test_host_rules(D):
    assert D._pair_bounds([0, 3, 7], 10).tolist() == [[0, 3, 3, 7], [0, 3, 7, 10], [3, 7, 7, 10]]
    assert D._pair_bounds([4], 10).shape == (0, 4) and D._neighbor_bounds([4], 10, True, 5).shape == (0, 4)
    # :272-275 with 40-locus and 3-locus neighbours: the first domain is cut to 2 * max(3, 5) loci, the second stays
    # and the second domain of the next pair to 2 * max(3, 5) loci
    assert D._neighbor_bounds([0, 40, 43], 60, True, 5).tolist() == [[30, 40, 40, 43], [40, 43, 43, 53]]
    assert D._neighbor_bounds([0, 40, 43], 60, True, 1).tolist() == [[34, 40, 40, 43], [40, 43, 43, 49]]
    assert D._neighbor_bounds([0, 40, 43], 60, False, 5).tolist() == [[0, 40, 40, 43], [40, 43, 43, 60]]
    assert list(D._contact_starts([7, 3, 10], 10)) == [0, 3, 7] and list(D._contact_starts([0, 4], 10)) == [0, 4]
    assert D._quads(7, [[3, 99, 5, 2]], 10).tolist() == [[7, 3, 10, 5, 5]]         # clipped as a slice clips; e < s is empty
    res = D._as_results(np.array([1.5, 0.0]), np.array([False, True]))
    assert type(res[0]) is np.float64 and type(res[1]) is int
    assert np.array(D._as_results(np.zeros(2), np.ones(2, bool))).dtype == np.array([0, 0]).dtype


def test_without_a_device_the_calls_raise(D):
    from imageanalysis3_amd import _lib
    if _lib.lib().ia3_init(0) == _lib.IA3_OK:
        assert not D._sliding_window_dist(np.zeros((4, 4)), 2).any()
        return
    with pytest.raises(_lib.IA3Error):
        D._sliding_window_dist(np.zeros((4, 4)), 2)
    with pytest.raises(_lib.IA3Error):
        D.domain_pdists(np.zeros((6, 3)), [0, 3])


def test_ctypes_mirrors_are_the_headers():
    from imageanalysis3_amd import _lib
    src = open(os.path.join(ROOT, "include", "ia3.h")).read()
    defines = {n: int(v) for n, v in re.findall(r"#define\s+(IA3_DOMAIN_[A-Z_]+)\s+(\d+)\s*$", src, flags=re.M)}
    assert len(defines) == 11 and all(getattr(_lib, n) == v for n, v in defines.items())
    assert _lib.DOMAIN_WINDOW_METRICS == {m: defines["IA3_DOMAIN_WINDOW_" + m.upper()] for m in K.WINDOW_METRICS}
    assert _lib.DOMAIN_DIST_METRICS == {m: defines["IA3_DOMAIN_DIST_" + m.upper()] for m in K.DIST_METRICS}
    hdr = open(os.path.join(ROOT, "imageanalysis3_amd", "csrc", "ia3_domain.h")).read()
    assert "hip/" not in hdr and "hip_runtime" not in hdr and "ia3_rt.h" not in hdr
    assert int(re.search(r"DM_MAX_WD = (\d+)", hdr).group(1)) == defines["IA3_DOMAIN_MAX_WINDOW"]
    assert int(re.search(r"DM_MAX_W = (\d+)", hdr).group(1)) == defines["IA3_DOMAIN_MAX_WINDOWS"]
    enums = dict(re.findall(r"(DM_[WD]_[A-Z_]+) = (\d+)", hdr))
    assert {k.replace("DM_W_", "IA3_DOMAIN_WINDOW_").replace("DM_D_", "IA3_DOMAIN_DIST_"): int(v) for k, v in enums.items()} \
        == {k: v for k, v in defines.items() if "_MAX_" not in k}
    for name in ("ia3_domain_create", "ia3_domain_free", "ia3_domain_slide_dev", "ia3_domain_dists_dev", "ia3_domain_contacts_dev"):
        assert name in _lib.PROTOTYPES and re.search(r"\b%s\(" % name, src)
    assert issubclass(_lib.DomainPopulation, _lib.Owner) and "free" not in vars(_lib.DomainPopulation)


# ---- csrc/ia3_domain.h on the host ----------------------------------------------------------------------------------------------

SRC = os.path.join(HERE, "native", "domain_cpu.cpp")
HDRS = [os.path.join(ROOT, "imageanalysis3_amd", "csrc", h) for h in ("ia3_domain.h", "ia3_distsum.h", "ia3_npsum.h", "ia3_order.h")]
EXE = os.path.join(HERE, "native", "domain_cpu")


def _build(exe, extra=()):
    if not os.path.isfile(exe) or os.path.getmtime(exe) < max(os.path.getmtime(p) for p in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off"] + list(extra) + ["-o", exe, SRC])
    return exe


def _records(gold):
    """The window maps with the fixture's rows, and the sets of domain pairs with the fixture's values."""
    from imageanalysis3_amd import _lib
    wp = K.window_populations()
    maps = [("win_lattice", 0, K.distance_map(wp["lattice"][0])), ("win_holes", 1, K.distance_map(wp["holes"][1])),
            ("win_short", 0, K.distance_map(wp["short"][0])), ("win_one", 1, K.distance_map(wp["one"][1])), ("win_map", 0, K.window_map())]
    w, n_win = [], 0
    for key, copy, mat in maps:
        rows = [(metric, wi) for metric in K.WINDOW_METRICS for wi in range(len(K.WDS))]
        w += [np.array([len(mat), len(rows)], dtype=np.float64), mat.ravel()]
        for metric, wi in rows:
            w += [np.array([_lib.DOMAIN_WINDOW_METRICS[metric], K.WDS[wi]], dtype=np.float64), gold["%s_%s" % (key, metric)][copy, wi]]
            n_win += len(mat)
    dp, norm = K.domain_populations(), K.normalization()
    ends = K.STARTS[1:] + [K.R_DOM]
    pairs = [((K.STARTS[i], ends[i]), (K.STARTS[j], ends[j])) for i in range(len(K.STARTS)) for j in range(i + 1, len(K.STARTS))]
    d, n_dist = [], 0

    def record(data, b1, b2, metric, allow, nmat, value):
        inter, intra = K.np_domain_sets(data, b1, b2, nmat)
        zero = isinstance(K.np_domain_distance(data, b1, b2, metric, nmat, allow), int)
        return [np.array([_lib.DOMAIN_DIST_METRICS[metric], allow, len(inter), len(intra), value, zero], dtype=np.float64), inter, intra]
    for name, copy, data in (("walk", 2, dp["walk"][2]), ("lattice", 0, dp["lattice"][0]), ("map", 0, K.domain_map())):
        for metric in K.DIST_METRICS:
            for allow in (0, 1):
                for nm, nmat in (("raw", None), ("norm", norm)):
                    if name == "lattice" and nm == "norm":
                        continue
                    values = gold["pd_%s_%s_%d_%s" % (name, metric, allow, nm)][copy]
                    for (b1, b2), value in zip(pairs, values):
                        d += record(data, b1, b2, metric, allow, nmat, value)
                        n_dist += 1
        single = [(b1, b2, metric, allow) for b1, b2 in K.SINGLE_CALLS for metric in K.DIST_METRICS for allow in (1, 0)]
        last = {"walk": dp["walk"][-1], "lattice": dp["lattice"][-1], "map": K.domain_map()}[name]
        for (b1, b2, metric, allow), value, zero in zip(single, gold["dd_%s_values" % name], gold["dd_%s_intzero" % name]):
            rec = record(last, b1, b2, metric, allow, None, value)
            assert rec[0][5] == float(zero)
            d += rec
            n_dist += 1
    return np.concatenate(w), n_win, np.concatenate(d), n_dist


def _check(exe, tmp_path, gold):
    w, n_win, d, n_dist = _records(gold)
    w.tofile(str(tmp_path / "windows.bin"))
    d.tofile(str(tmp_path / "dists.bin"))
    p = subprocess.run([exe, str(tmp_path / "windows.bin"), str(tmp_path / "dists.bin")], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       universal_newlines=True)
    assert p.returncode == 0, p.stdout + p.stderr
    m = re.search(r"windows (\d+) mismatches (\d+)", p.stdout)
    assert m and int(m.group(1)) == n_win > 3000 and int(m.group(2)) == 0
    m = re.search(r"dists (\d+) mismatches (\d+)", p.stdout)
    assert m and int(m.group(1)) == n_dist > 300 and int(m.group(2)) == 0


def test_windows_and_selects_on_the_host(tmp_path, gold):
    _check(_build(EXE), tmp_path, gold)


def test_windows_and_selects_under_sanitizers(tmp_path, gold):
    """the same stand-alone program with AddressSanitizer and UBSan (a host program of its own: nothing is preloaded)"""
    _check(_build(EXE + "_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]), tmp_path, gold)
