"""No GPU: the reference's names and signatures of spot_tools/scoring.py, the refusals that come before any device call, the
host one-liners against the fixture (tests/golden/scoring.npz, the reference's own outputs), the ctypes mirrors against
include/ia3.h, and the stand-alone check of csrc/ia3_score.h and of the any-length pairwise sum (tests/native/score_cpu.cpp):
the serial text that score.hip runs per lane, against the fixture's distances, references and _cum_prob values and against
np.add.reduce for every length from 1 to 5000, also under AddressSanitizer and UBSan."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import load_golden
from harness import scoring_cases as K

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def gold():
    return load_golden("scoring.npz")


@pytest.fixture(scope="module")
def S():
    from imageanalysis3_amd.spot_tools import scoring
    return scoring


@pytest.fixture()
def no_device(monkeypatch):
    """Any call into the library fails the test: the errors below come before it."""
    from imageanalysis3_amd import _lib

    def refuse():
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "lib", refuse)
    return _lib


def _outputs(gold, key):
    out = []
    while "%s__%d" % (key, len(out)) in gold:
        out.append(gold["%s__%d" % (key, len(out))])
    return out


def test_signatures_are_the_references(S, gold):
    for name in K.SIGNATURE_NAMES:
        assert str(inspect.signature(getattr(S, name))) == str(gold["sig_" + name]), name


def test_fixture_holds_what_the_cases_need(gold):
    assert os.path.getsize(os.path.join(HERE, "golden", "scoring.npz")) < 400000
    keys = set(k for k, _ in K.fixture_calls())
    assert keys == set(k.rsplit("__", 1)[0] for k in gold if not k.startswith("sig_"))
    pop = K.population()
    assert [len(p["cand"]) for p in pop][:3] == [1, 65, 130] and len(pop[0]["sel"]) == 1
    # odd and even medians with ties, both one-sided neighbourhoods, the four fallbacks, a raise for a reference without values
    fwd, rev = gold["geo3_nb__0"], gold["geo3_nb__1"]
    assert (np.isnan(fwd) & np.isnan(rev)).any() and (~np.isnan(fwd) & np.isnan(rev)).any() and (~np.isnan(fwd) & ~np.isnan(rev)).any()
    assert [gold["ref7_cdf_1__%d" % a].tolist() for a in range(4)] == [[1000], [np.inf], [np.inf], [1.]]
    assert str(gold["css7_keepnan__0"]).startswith("ValueError") and str(gold["css_list_dzxy__0"]).startswith("TypeError")
    assert (gold["geo8_fw__0"] == 0).sum() >= 4                  # ties at vmin = 0
    assert np.isnan(gold["geo5_lc5__0"]).any() and not np.isnan(gold["geo5_lc33__0"]).all()
    assert (gold["css6_plain__3"] == -1000).any() and np.isneginf(gold["css1_plain__0"]).any()
    assert not gold["css1_degen__0"].any() and gold["css1_degen__1"].any()


def test_host_functions_equal_the_fixture(S, gold, no_device):
    for name, fn, args, kw in K.host_cases():
        got = getattr(S, fn)(*args, **kw)
        assert K.same(got, gold["val_%s__0" % name]), name
    spots = K.population()[6]["cand"].copy()
    before = spots.copy()
    S._filter_intensities(spots, intensity_th=K.TH)
    assert K.same(spots, before)                                  # np.array copies: the caller's table stays
    assert isinstance(S.radius_of_gyration(np.zeros(3)), IndexError) and str(gold["rg_1d__0"]) == "IndexError"
    p = K.population()[1]
    assert K.same(S._center_distance(K.zxys(p["cand"])[0], K.zxys(p["sel"])[0]), gold["ct_1d__0"])


def test_not_built_names_say_so(S, no_device):
    with pytest.raises(NotImplementedError, match="not built"):
        S.generate_cdf_scores([1.], [1., 2.])
    with pytest.raises(NotImplementedError, match="not built"):
        S.Normalize_Intensities(np.zeros((2, 4)), np.zeros((2, 4)))


def test_refusals_come_before_the_device(S, gold, no_device):
    L = no_device
    p = K.population()[1]
    z, ids = K.zxys(p["cand"]), p["cand_ids"]
    # the reference's own errors, with its words where the fixture recorded them
    for key, f in K.other_calls():
        want = _outputs(gold, key)
        if want[0].dtype.kind == 'U' and ":" in str(want[0]) and key != "ssc_rg":   # that one is float() of a device result
            got = f(S)
            assert str(got[0]) == str(want[0]), key
    with pytest.raises(ValueError, match="not enough values"):
        S.distance_score([1., 2.], [np.nan], metric='cdf')
    with pytest.raises(ValueError, match="has not been supported yet"):
        S.distance_score([1., 2.], [1.], metric='other')
    with pytest.raises(ValueError, match="should be an array rather than one value"):
        S.intensity_score([1., 2.], 3., metric='cdf')
    with pytest.raises(ValueError, match="no valid points at all"):
        S._cum_prob([np.nan], [1.])
    with pytest.raises(IndexError, match="Wrong shape for spot_zxys"):
        S._center_distance(np.zeros((2, 2, 3)))
    with pytest.raises(IndexError, match="Wrong input "):
        S.generate_ref_from_chromosome(p["sel"], [1, 2], K.DZXY)
    with pytest.raises(TypeError):
        S.generate_ref_from_chromosome(p["sel"])                 # the package's distance_zxy is a list
    with pytest.raises(ValueError, match="Not supported yet!"):
        S.generate_ref_from_chromosome(p["sel"], None, K.DZXY, ref_dist_metric='ks')
    with pytest.raises(TypeError, match="Wrong input type for spot_ids"):
        S.spot_score_in_chromosome(p["cand"], "ids", p["sel"], distance_zxy=K.DZXY)
    with pytest.raises(IndexError, match="length should match"):
        S.spot_score_in_chromosome(p["cand"], ids[:3], p["sel"], distance_zxy=K.DZXY)
    with pytest.raises(IndexError, match="length should match"):
        S.spot_score_in_chromosome(p["cand"], ids, p["sel"], [1, 2], distance_zxy=K.DZXY)
    with pytest.raises(IndexError, match="Wrong shape of _spots"):
        S.chromosomal_spot_scores(p["cand"][0], ids, p["sel"], distance_zxy=K.DZXY)
    with pytest.raises(IndexError, match="Wrong shape of _sel_spots"):
        S.chromosomal_spot_scores(p["cand"], ids, p["sel"][0], distance_zxy=K.DZXY)
    with pytest.raises(TypeError, match="Wrong input type for region_ids"):
        S.chromosomal_spot_scores(p["cand"], None, p["sel"], distance_zxy=K.DZXY)
    with pytest.raises(ValueError, match="Not supported yet!"):
        S.chromosomal_spot_scores(p["cand"], ids, p["sel"], score_metric='linear', distance_zxy=K.DZXY, verbose=False)
    # above the built limits
    many = np.zeros(L.IA3_SCORE_MAX_PER_REGION + 1, dtype=int)
    zz = np.zeros((len(many), 3))
    with pytest.raises(NotImplementedError, match="of one region"):
        S.neighboring_distances(zz, many)
    with pytest.raises(NotImplementedError, match="of one region"):
        S._local_distance(z, ids, zz, many)
    with pytest.raises(NotImplementedError, match="of one region"):
        S.chromosomal_spot_scores(np.zeros((len(many), 4)), many, p["sel"], distance_zxy=K.DZXY, verbose=False)
    with pytest.raises(NotImplementedError, match="of one region"):
        S.chromosomal_spot_scores(p["cand"], ids, np.zeros((len(many), 4)), many, distance_zxy=K.DZXY, verbose=False)
    assert L.score_table([np.zeros((L.IA3_SCORE_MAX_PER_REGION, 4))], [many[:-1]], "candidate")[2].tolist() == [0, 64]
    with pytest.raises(NotImplementedError, match="local_size"):
        S._local_distance(z, ids, z, ids, local_size=L.IA3_SCORE_MAX_LOCAL + 2)
    assert L.score_half(L.IA3_SCORE_MAX_LOCAL + 1) == 16 and L.score_half(0) == 0 and L.score_half(6) == 2
    with pytest.raises(IndexError):
        S._local_distance(z, ids, z, ids, local_size=-1)         # np.delete of an empty range, as in the reference
    with pytest.raises(ValueError, match="outside int32"):
        S.neighboring_distances(z[:2], [0, 2**31])
    with pytest.raises(ValueError):
        L.ScorePopulation.upload([], [], [], [])
    with pytest.raises(ValueError, match="has no selected spot"):
        L.ScorePopulation.upload([p["cand"]], [ids], [np.zeros((0, 4))], None)
    with pytest.raises(ValueError):
        L.ScorePopulation.upload([p["cand"]], [ids], [p["sel"], p["sel"]], None)
    with pytest.raises(ValueError):
        L.ScorePopulation.upload([p["cand"]], [ids], [p["sel"]], None, chr_centers=[None, None])
    with pytest.raises(ValueError):
        L.ScorePopulation.upload([p["cand"]], [ids], [p["sel"]], None, distance_zxy=[1, 2])
    # a population without a handle: what its methods refuse
    pop = L.ScorePopulation(None, ids, np.array([0, len(ids)], dtype=np.int32), np.array([0, len(p["sel"])], dtype=np.int32))
    with pytest.raises(ValueError, match="Not supported yet!"):
        pop.references('ks')
    with pytest.raises(NotImplementedError):
        pop.references('median', local_size=40)
    with pytest.raises(NotImplementedError):
        pop.geometry(local_size=40)
    with pytest.raises(ValueError):
        pop.scores('ks')
    with pytest.raises(ValueError):
        pop.scores('cdf', 'median')
    with pytest.raises(ValueError):
        pop.scores('cdf', weights=(1, 1, 1))
    with pytest.raises(ValueError):
        pop.replace_selected([p["sel"], p["sel"]])
    with pytest.raises(NotImplementedError):
        pop.replace_selected([np.zeros((len(many), 4))], [many])
    with pytest.raises(ValueError, match="Not supported yet!"):
        S.population_chromosomal_spot_scores(pop, 'linear')
    with pytest.raises(ValueError):
        S.population_score_references(pop, ref_dist_metric='ks')


def test_bindings_mirror_the_header():
    from imageanalysis3_amd import _lib
    src = open(os.path.join(ROOT, "include", "ia3.h")).read()
    defines = {n: int(v) for n, v in re.findall(r"#define\s+(IA3_SCORE_[A-Z0-9_]+)\s+(-?\d+)\s*$", src, flags=re.M)}
    assert len(defines) == 11 and all(getattr(_lib, n) == v for n, v in defines.items())
    assert {k: v for k, v in _lib.SCORE_REF_METRICS.items()} == {n[len("IA3_SCORE_REF_"):].lower(): v for n, v in defines.items() if "_REF_" in n}
    for name in ("ia3_score_create", "ia3_score_replace_selected", "ia3_score_free", "ia3_score_refs_dev", "ia3_score_scores_dev",
                 "ia3_score_values_dev", "ia3_score_neighbor_lists_dev"):
        assert name in _lib.PROTOTYPES and re.search(r"\b%s\(" % name, src)
    assert issubclass(_lib.ScorePopulation, _lib.Owner) and "free" not in vars(_lib.ScorePopulation)
    hdr = open(os.path.join(ROOT, "imageanalysis3_amd", "csrc", "ia3_score.h")).read()
    assert "hip/" not in hdr and "SC_MAX_PER_REGION = %d" % _lib.IA3_SCORE_MAX_PER_REGION in hdr and "SC_MAX_LOCAL = %d" % _lib.IA3_SCORE_MAX_LOCAL in hdr


# ---- csrc/ia3_score.h on the host -----------------------------------------------------------------------------------------------

SRC = os.path.join(HERE, "native", "score_cpu.cpp")
HDRS = [os.path.join(ROOT, "imageanalysis3_amd", "csrc", h) for h in ("ia3_score.h", "ia3_domain.h", "ia3_distsum.h", "ia3_npsum.h", "ia3_order.h",
                                                                       "ia3_model.h")]
EXE = os.path.join(HERE, "native", "score_cpu")


def _build(exe, extra=()):
    if not os.path.isfile(exe) or os.path.getmtime(exe) < max(os.path.getmtime(p) for p in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off"] + list(extra) + ["-o", exe, SRC])
    return exe


def _records(gold):
    from imageanalysis3_amd import _lib
    rng = np.random.default_rng(77)
    a = rng.normal(size=5000) * np.exp(rng.normal(size=5000) * 3.)
    rec = [np.array([1., len(a)]), a, np.array([np.add.reduce(a[:n]) for n in range(1, len(a) + 1)])]
    counts = dict(sums=len(a), geometry=0, references=0, values=0)
    for c, p in enumerate(K.population()):
        ctr = np.zeros(3) if p["center"] is None else p["center"]
        rec += [np.array([2., len(p["cand"]), len(p["sel"]), 0. if p["center"] is None else 1.]), ctr, K.DZXY, np.array([K.TH]),
                p["cand"].ravel(), p["cand_ids"].astype(np.float64), p["sel"].ravel(), p["sel_ids"].astype(np.float64)]
        rec += [np.array([10.]), gold["geo%d_ct__0" % c]]
        for ls in K.LOCAL_SIZES:
            rec += [np.array([11., _lib.score_half(ls)]), gold["geo%d_lc%d__0" % (c, ls)]]
        rec += [np.array([12.]), gold["geo%d_nb__0" % c], gold["geo%d_nb__1" % c]]
        counts["geometry"] += len(p["cand"]) * (2 + len(K.LOCAL_SIZES))
        for metric in K.REF_METRICS:
            for ign in (1, 0):
                out = [np.atleast_1d(np.asarray(o, dtype=np.float64)) for o in _outputs(gold, "ref%d_%s_%d" % (c, metric, ign))]
                assert len(out) == 4
                rec += [np.array([13., _lib.SCORE_REF_METRICS[metric], ign] + [len(o) for o in out], dtype=np.float64)] + out
                counts["references"] += sum(len(o) for o in out)
        rec.append(np.zeros(1))
    kinds = {"_cum_prob": _lib.IA3_SCORE_KIND_CUM_PROB, "distance_score": _lib.IA3_SCORE_KIND_DIST_LINEAR}
    for name, fn, args, kw in K.value_cases():
        want = gold["val_%s__0" % name]
        if not (name.startswith("cum_") or name.startswith("dlin_")) or want.dtype.kind == 'U':
            continue
        if fn == "_cum_prob":
            ref, x, scalar, lo, hi = np.asarray(args[0], dtype=np.float64), args[1], 0., kw.get("vmin", -np.inf), kw.get("vmax", np.inf)
        else:
            lim = kw.get("distance_limits", [-np.inf, np.inf])
            ref, x, scalar, lo, hi = np.zeros(0), args[0], float(args[1]), min(lim), max(lim)
        x = np.atleast_1d(np.asarray(x, dtype=np.float64)).ravel()
        rec += [np.array([3., kinds[fn], len(ref), len(x), kw.get("weight", 1.), lo, hi, scalar, kw.get("nan_mask", -1000)], dtype=np.float64),
                ref, x, want.ravel()]
        counts["values"] += len(x)
    return np.concatenate([np.asarray(r, dtype=np.float64).ravel() for r in rec]), counts


def _check(exe, tmp_path, gold):
    rec, counts = _records(gold)
    rec.tofile(str(tmp_path / "records.bin"))
    p = subprocess.run([exe, str(tmp_path / "records.bin")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert p.returncode == 0, p.stdout + p.stderr
    m = re.search(r"sums (\d+) geometry (\d+) references (\d+) values (\d+) mismatches (\d+)", p.stdout)
    assert m, p.stdout
    assert [int(g) for g in m.groups()] == [counts["sums"], counts["geometry"], counts["references"], counts["values"], 0]
    assert counts["sums"] == 5000 and counts["geometry"] > 2500 and counts["references"] > 1500 and counts["values"] > 500


def test_serial_forms_on_the_host(tmp_path, gold):
    _check(_build(EXE), tmp_path, gold)


def test_serial_forms_under_sanitizers(tmp_path, gold):
    """the same stand-alone program with AddressSanitizer and UBSan (a host program of its own: nothing is preloaded)"""
    _check(_build(EXE + "_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]), tmp_path, gold)
