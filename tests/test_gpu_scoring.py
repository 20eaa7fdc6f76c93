"""GPU: the chromosomal spot scores on the device (csrc/score.hip) against the reference's own outputs
(tests/golden/scoring.npz) through the reference-named functions and the flat forms on a resident population.

Every finite value, infinity and zero equals the reference's in every bit; a NaN stands where the reference has a NaN.
Every call runs twice and every chromosome alone and in the batch, and the bytes are compared; an exception of the
reference is raised with the reference's words."""
import numpy as np
import pytest

from conftest import load_golden
from harness import scoring_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from imageanalysis3_amd import _lib
    _lib.check(_lib.lib().ia3_init(0))
    return _lib


@pytest.fixture(scope="module")
def S(L):
    from imageanalysis3_amd.spot_tools import scoring
    return scoring


@pytest.fixture(scope="module")
def gold():
    return load_golden("scoring.npz")


def _outputs(gold, key):
    out = []
    while "%s__%d" % (key, len(out)) in gold:
        out.append(gold["%s__%d" % (key, len(out))])
    return out


def _is_error(want):
    return want[0].dtype.kind == 'U' and ":" in str(want[0])


def _bytes(arrays):
    return [np.asarray(a).tobytes() for a in arrays]


def _equal(got, want, key):
    assert len(got) == len(want), key
    for i, (g, w) in enumerate(zip(got, want)):
        if w.dtype.kind == 'U':
            assert str(g) == str(w), (key, i)
        else:
            g = np.asarray(g, dtype=np.float64)
            assert g.shape == w.shape, (key, i, g.shape, w.shape)
            assert K.same(g, w), (key, i, np.argwhere(~((g == w) | (np.isnan(g) & np.isnan(w))))[:5].tolist())


def _upload(L, chroms, selected=None):
    sel = [(p["sel"], p["sel_ids"]) for p in chroms] if selected is None else selected
    return L.ScorePopulation.upload([p["cand"] for p in chroms], [p["cand_ids"] for p in chroms], [s for s, _ in sel], [i for _, i in sel],
                                    [p["center"] for p in chroms], K.DZXY)


def test_reference_named_functions_equal_the_reference(S, gold, capsys):
    for key, f in K.fixture_calls():
        got, again = f(S), f(S)
        assert _bytes(got) == _bytes(again), key
        _equal(got, _outputs(gold, key), key)
    capsys.readouterr()


def test_reference_types_are_the_references(S, capsys):
    p = K.population()[7]
    r = S.generate_ref_from_chromosome(p["sel"], p["sel_ids"], K.DZXY, intensity_th=K.TH, ref_dist_metric='cdf')
    assert r[0] == [1000] and type(r[0]) is list and r[1] == [np.inf] and r[2] == [np.inf] and isinstance(r[3], np.ndarray) and r[3].tolist() == [1.]
    assert "_ct_dist has no valid values in this chromosome" in capsys.readouterr().out
    p = K.population()[1]
    r = S.generate_ref_from_chromosome(p["sel"], p["sel_ids"], K.DZXY, ref_dist_metric='median')
    assert all(type(v) is np.float64 for v in r)
    r = S.generate_ref_from_chromosome(p["sel"], p["sel_ids"], K.DZXY, ref_dist_metric='rg')
    assert type(r[0]) is np.float64 and r[0] == r[1] == r[2] and isinstance(r[3], np.ndarray)
    spots = p["cand"].copy()
    S.chromosomal_spot_scores(spots, p["cand_ids"], p["sel"], p["sel_ids"], distance_zxy=K.DZXY, verbose=False)
    assert K.same(spots, p["cand"])


def test_population_scores_equal_the_reference(L, S, gold):
    chroms = K.population()
    for variant, _ in K.SCORE_VARIANTS:
        kw = K.score_kwargs(variant)
        want = [_outputs(gold, "css%d_%s" % (c, variant)) for c in range(len(chroms))]
        good = [c for c in range(len(chroms)) if not _is_error(want[c])]
        assert len(good) >= 6
        with _upload(L, [chroms[c] for c in good]) as pop:
            got = S.population_chromosomal_spot_scores(pop, **kw)
            again = S.population_chromosomal_spot_scores(pop, **kw)
        for k, c in enumerate(good):
            assert _bytes(got[k]) == _bytes(again[k]), (variant, c)
            _equal(list(got[k]), want[c], (variant, c))
        for c in range(len(chroms)):
            with _upload(L, [chroms[c]]) as one:
                if c in good:
                    assert _bytes(S.population_chromosomal_spot_scores(one, **kw)[0]) == _bytes(got[good.index(c)]), (variant, c)
                else:
                    with pytest.raises(ValueError) as e:
                        S.population_chromosomal_spot_scores(one, **kw)
                    assert "ValueError: %s" % e.value == str(want[c][0]), (variant, c)
        if len(good) < len(chroms):
            with _upload(L, chroms) as pop, pytest.raises(ValueError):
                S.population_chromosomal_spot_scores(pop, **kw)


def test_population_references_equal_the_reference(L, S, gold):
    chroms = K.population()
    with _upload(L, chroms) as pop:
        alone = [_upload(L, [p]) for p in chroms]
        for metric in K.REF_METRICS:
            for ign in (True, False):
                got = S.population_score_references(pop, K.TH, 5, metric, ign)
                again = S.population_score_references(pop, K.TH, 5, metric, ign)
                for c in range(len(chroms)):
                    assert _bytes(got[c]) == _bytes(again[c]), (metric, ign, c)
                    _equal(list(got[c]), _outputs(gold, "ref%d_%s_%d" % (c, metric, ign)), (metric, ign, c))
                    assert _bytes(S.population_score_references(alone[c], K.TH, 5, metric, ign)[0]) == _bytes(got[c]), (metric, ign, c)
        for one in alone:
            one.free()


def test_linear_scores_on_a_population(L, S, gold):
    """The linear metric against median references in one call, put together as spot_score_in_chromosome does (:387-395)."""
    chroms = K.population()
    with _upload(L, chroms) as pop:
        val, cls, _ = pop.scores('linear', 'median', 5, K.TH, True, (1., 0.1, 1., 1.), [0, 500])
        val2, cls2, _ = pop.scores('linear', 'median', 5, K.TH, True, (1., 0.1, 1., 1.), [0, 500])
    assert val.tobytes() == val2.tobytes() and cls.tobytes() == cls2.tobytes()
    parts = []
    for a in (0, 1):
        s = val[a].copy()
        assert not (cls[a] & 3).any()
        s[(cls[a] & L.SCORE_NAN_IN) != 0] = -3.
        parts.append(s)
    s = S._finish(val[3], cls[3], 1., val[3].shape)
    s[np.isnan(s)] = -3.
    s[np.isinf(s)] = -1000.
    total = parts[0] + parts[1] + s
    for c in range(len(chroms)):
        assert K.same(total[pop.cand_start[c]:pop.cand_start[c + 1]], gold["ssc%d_linear_median__0" % c]), c


def test_replace_selected_equals_a_fresh_upload(L, S):
    chroms = K.population()
    kw = K.score_kwargs("lim500")
    with _upload(L, chroms[:7]) as fresh:
        want = S.population_chromosomal_spot_scores(fresh, **kw)
        want_refs = S.population_score_references(fresh, K.TH, 5, 'mean', True)
    with _upload(L, chroms[:7], [(p["cand"], p["cand_ids"]) for p in chroms[:7]]) as pop:
        first = S.population_chromosomal_spot_scores(pop, **kw)
        assert any(_bytes(a) != _bytes(b) for a, b in zip(first, want))
        pop.replace_selected([p["sel"] for p in chroms[:7]], [p["sel_ids"] for p in chroms[:7]])
        assert pop.S == sum(len(p["sel"]) for p in chroms[:7])
        got = S.population_chromosomal_spot_scores(pop, **kw)
        got_refs = S.population_score_references(pop, K.TH, 5, 'mean', True)
    for c in range(7):
        assert _bytes(got[c]) == _bytes(want[c]) and _bytes(got_refs[c]) == _bytes(want_refs[c]), c


def test_the_library_refuses_what_is_not_built(L):
    p = K.population()[1]
    cand, ids = np.ascontiguousarray(p["cand"][:, :4]), p["cand_ids"].astype(np.int64)
    start = np.array([0, len(ids)], dtype=np.int32)
    dz = K.DZXY.copy()
    import ctypes as C

    def create(cand_ids, cand_start):
        h = C.c_void_p()
        rc = L.lib().ia3_score_create(L.ptr(cand.reshape(-1)), L.ptr(cand_ids), L.ptr(cand_start), L.ptr(cand.reshape(-1)), L.ptr(ids), L.ptr(start),
                                      None, None, 1, L.ptr(dz), C.byref(h))
        assert h.value is None or rc == L.IA3_OK
        if rc == L.IA3_OK:
            L.lib().ia3_score_free(h)
        return rc
    assert create(ids, start) == L.IA3_OK
    assert create(np.zeros(len(ids), dtype=np.int64), start) == L.IA3_EINVAL            # 65 rows of one region
    far = ids.copy()
    far[3] = 2**31
    assert create(far, start) == L.IA3_EINVAL
    assert create(ids, np.array([0, 0], dtype=np.int32)) == L.IA3_EINVAL                 # an empty chromosome
    with _upload(L, [p]) as pop:
        geom = np.empty((5, pop.N))
        assert L.lib().ia3_score_scores_dev(pop._h, -1, 0, 17, 1, 0., 0., 1, None, 0., 0., L.ptr(geom.reshape(-1)), None, None, None) == L.IA3_EINVAL
        assert L.lib().ia3_score_scores_dev(pop._h, 1, 0, 2, 1, 0., 0., 1, None, 0., 0., None, None, None, None) == L.IA3_EINVAL
        cnt, scal = np.empty((1, 4), dtype=np.int32), np.empty((1, 4))
        assert L.lib().ia3_score_refs_dev(pop._h, 9, 2, 0., 1, None, L.ptr(cnt.reshape(-1)), L.ptr(scal.reshape(-1))) == L.IA3_EINVAL
        assert L.lib().ia3_score_refs_dev(None, 0, 2, 0., 1, None, L.ptr(cnt.reshape(-1)), L.ptr(scal.reshape(-1))) == L.IA3_EINVAL
