"""No GPU: the statement of the population picker (tests/harness/pick_ref.py) against the reference's own outputs
(tests/golden/pick.npz), the search-node enumeration behind the device's log tables against the literal ``cum_val``, NumPy's
two norm forms and its ``nanmean`` order, and the shims' argument handling that needs no device."""
import numpy as np
import pytest

from conftest import load_golden
from harness import pick_cases as K
from harness import pick_ref as R


@pytest.fixture(scope="module")
def gold():
    return load_golden("pick.npz")


@pytest.fixture(scope="module")
def PK():
    from imageanalysis3_amd.spot_tools import picking
    return picking


_records = {}


def record(name):
    """The statement's flow of a case, made once: brightest picks, E-step, M-step against them, difference."""
    if name not in _records:
        c = K.case(name)
        picks0, idx0 = R.pick_by_intensity(c["cands"])
        split = c["split_int"] or c["split_dist"]
        e = R.e_step(picks0, c["ids"], picks0, c["ids"], c["neighbor_len"], c["channels"], split, None)
        m = R.m_step(c["cands"], c["ids"], picks0, c["ids"], e["sorted"], c["neighbor_len"], c["center_weight"],
                     c["local_weight"], c["channels"], c["split_int"], c["split_dist"], c["centers"])
        _records[name] = dict(picks0=picks0, idx0=idx0, e=e, m=m, diff=R.difference(picks0, m["picks"]))
    return _records[name]


def stored(rec):
    out = dict(picks0=rec["picks0"], e_ct=rec["e"]["ct"], e_lc=rec["e"]["lc"], cdist=rec["m"]["cdist"], mids=rec["m"]["mids"],
               scores=rec["m"]["scores"], picks=rec["m"]["picks"], sel_scores=rec["m"]["sel_scores"])
    for kind in R.KINDS:
        for key, v in rec["e"]["sorted"][kind].items():
            out["sorted_%s_%s" % (kind, key)] = v
    return out


@pytest.mark.parametrize("name", list(K.CASES))
def test_statement_equals_the_reference(gold, name):
    """Byte for byte (NaNs as NaNs): scores and picks against the stored arrays, every array against its stored digest."""
    rec, meta = record(name), K.golden_meta(gold, name)
    assert rec["m"]["pick_idx"].astype(np.int8).tobytes() == gold[name + "_pick_idx"].tobytes()
    assert list(rec["diff"]) == meta["diff"]
    for kind in R.KINDS:
        assert [str(k) for k in rec["e"]["sorted"][kind]] == meta["keys"][kind]
        assert [len(v) for v in rec["e"]["sorted"][kind].values()] == meta["lengths"][kind]
    mine = stored(rec)
    assert sorted(mine) == sorted(meta["digests"])
    for key, v in mine.items():
        assert R.digest(v) == meta["digests"][key], (name, key)
        if name != "big" and key in ("scores", "sel_scores", "picks"):
            assert R.same_bits(v, gold["%s_%s" % (name, key)]), (name, key)


def test_1d_rows_take_another_norm_than_their_table_twins():
    """The 1-D rows of the case were chosen so that both of their distances differ in the last bit between the two norm
    forms: results made without the per-entry flag are not the reference's."""
    c, rec = K.case("one_d"), record("one_d")
    plain = R.m_step(K.tables_only(c["cands"]), c["ids"], rec["picks0"], c["ids"], rec["e"]["sorted"], c["neighbor_len"],
                     c["center_weight"], c["local_weight"])
    rows = [K.first_row(c["cands"], p, r) for (p, r) in K.ONE_D_ROWS]
    for k in rows:
        assert rec["m"]["cdist"][k, 0] != plain["cdist"][k, 0] and rec["m"]["cdist"][k, 1] != plain["cdist"][k, 1]
    other = np.setdiff1d(np.arange(len(plain["cdist"])), rows)
    assert R.same_bits(rec["m"]["cdist"][other], plain["cdist"][other])
    # the twin of the first row, a 1 x 4 table in another chromosome, is the same spot
    twin = K.first_row(c["cands"], 1, 4)
    assert R.same_bits(np.asarray(c["cands"][1][4])[0], np.asarray(c["cands"][0][4]))
    assert not np.isnan(rec["m"]["cdist"][[twin] + rows]).any()


@pytest.mark.parametrize("n", K.CUM_SIZES)
def test_search_nodes_against_the_literal_cum_val(n):
    from imageanalysis3_amd import _lib
    v, targets = K.cum_table(n)
    mids = R.search_nodes(n)
    lib_mids = _lib.pick_search_nodes(n)
    assert len(lib_mids) <= 1 << 16 and (lib_mids[0] == -1)
    k = min(len(mids), len(lib_mids))
    assert (mids[:k] == lib_mids[:k]).all() and (mids[k:] == -1).all() and (lib_mids[k:] == -1).all()
    lo, lo1 = _lib.pick_log_tables(n)
    for t in targets:
        mid, node = R.search_node(v, t)
        assert mid == R.cum_val_mid(v, t) == lib_mids[node], (n, t)
        val = R.cum_val(v, t)
        assert np.float64(np.log(val)).tobytes() == lo[node].tobytes()
        assert np.float64(np.log(1 - val)).tobytes() == lo1[node].tobytes()
    if n == 300001:   # the 16-iteration stop: some search ends with an interval that is still open
        assert (mids >= 0).sum() == (1 << 16) - 1


def test_search_nodes_of_an_empty_array():
    from imageanalysis3_amd import _lib
    with pytest.raises(IndexError):
        _lib.pick_search_nodes(0)
    with pytest.raises(IndexError):
        R.cum_val([], 1.0)


def test_norm_forms_equal_numpy():
    rs = np.random.RandomState(0)
    d = rs.uniform(-3000, 3000, (5000, 3))
    rows = np.linalg.norm(d, axis=1)
    assert int((R.norm_rows(d) != rows).sum()) == 0
    vec = np.array([np.linalg.norm(v) for v in d])
    mine = np.array([R.norm_vec(v) for v in d])
    assert int((mine != vec).sum()) == 0
    # the two forms are not the same function: the per-entry flag is needed
    assert int((rows != vec).sum()) > 0


def test_nanmean_adds_rows_in_order():
    rs = np.random.RandomState(1)
    for n in (1, 2, 14, 300, 1301):     # 1301 rows: more than any chromosome of the fixtures holds
        t = rs.uniform(0, 20000, (n, 4))
        t[rs.rand(n, 4) < 0.1] = np.nan
        assert R.same_bits(R.nanmean(t), R.nanmean_loop(t)), n
    assert np.isnan(R.nanmean_loop(np.full((3, 4), np.nan))).all()


def test_windows_equal_the_statement(PK):
    for name in K.SMALL:
        c = K.case(name)
        for split in (False, True):
            if split and (c["channels"] is None or len(c["ids"]) < 2):
                continue
            ws, wi = PK._windows(c["ids"], c["ids"], c["neighbor_len"], c["channels"], split)
            for j, cid in enumerate(c["ids"]):
                assert list(wi[ws[j]:ws[j + 1]]) == R.window(cid, c["ids"], c["neighbor_len"], c["channels"], j, split)
    # a split window without any id in reach does not index in the reference
    with pytest.raises(IndexError):
        PK._windows([0], [0], 2, ["750"], True)
    ws, wi = PK._windows([0], [0], 2, None, False)
    assert list(ws) == [0, 0] and len(wi) == 0


def test_pack_and_host_shims(PK):
    c = K.case("one_d")
    table, start, flags, P, Rn = PK._pack(c["cands"])
    assert (P, Rn) == (3, 9) and start[-1] == len(table) and flags.sum() == 2 and flags[4] == 1 and flags[9 + 4] == 0
    assert R.same_bits(table[start[4]], np.asarray(c["cands"][0][4]))
    ints = PK.extract_intensities(c["cands"][0])
    assert ints[2] == [] and ints[4] == c["cands"][0][4][0] and np.array_equal(ints[0], c["cands"][0][0][:, 0])
    spots = [np.array([[10., 1, 2, 3, 5, 9], [20., 2, 3, 4, 4, 9]]), [], np.array([30., 3, 4, 5, 6, 9])]
    out = PK.convert_spots_to_hzxys(spots, pix_size=[200, 100, 100], normalize_spot_background=True)
    assert np.array_equal(out[0], [[2., 200, 200, 300], [5., 400, 300, 400]]) and out[1] == []
    assert np.array_equal(out[2], [5., 600, 400, 500]) and spots[0][0, 1] == 1
    v = np.array([1., 2., np.nan, 4.])
    assert PK.slow_cum_val(v, 3.) == 2 / 3


def test_shim_errors_that_need_no_device(PK, gold):
    c = K.case("base")
    cands = K.tables_only(c["cands"])
    assert str(gold["raises_unbound"]) == "UnboundLocalError"
    with pytest.raises(UnboundLocalError):
        PK.pick_spots_by_scores(cands, c["ids"], verbose=False)
    with pytest.raises(ValueError):
        PK.pick_spots_by_scores(cands, c["ids"], split_intensity_channels=True, verbose=False)
    with pytest.raises(ValueError):
        PK.pick_spots_by_scores(cands, c["ids"], split_distance_channels=True, verbose=False)
    with pytest.raises(NotImplementedError):
        PK.pick_spots_by_scores(cands, c["ids"], ref_channels=K.CHANNELS3 * 3, split_intensity_channels=True,
                                collapse_regions=False, verbose=False)
    picks0 = record("base")["picks0"]
    with pytest.raises(NotImplementedError):
        PK.generate_reference_from_population(picks0, split_channels=False, collapse_regions=False, verbose=False)
    with pytest.raises(ValueError):
        PK.generate_reference_from_population(picks0, verbose=False)                      # split_channels defaults to True
    with pytest.raises(IndexError):
        PK.generate_reference_from_population(picks0, ref_channels=["750"], verbose=False)
    with pytest.raises(NotImplementedError):
        PK.EM_pick_scores_in_population(cands)
    with pytest.raises(NotImplementedError):
        PK.chromosome_center_dists(cands[0], ref_center={"all": [1, 2, 3]})
    with pytest.raises(ValueError):
        PK.chromosome_center_dists(cands[0], split_channels=True)
    with pytest.raises(ValueError):
        PK.chromosome_center_dists(cands[0], ref_channels=["750"])
    with pytest.raises(TypeError):
        PK.chromosome_center_dists(cands[0], ref_center=5.0)
    with pytest.raises(IndexError):
        PK.chromosome_center_dists(cands[0], ref_center=[1.0, 2.0])
    with pytest.raises(IndexError):
        PK.local_center_dists(cands[0], [0, 1], picks0[0])
    with pytest.raises(AttributeError):
        PK.local_center_dists(cands[0], 3, picks0[0])
    with pytest.raises(NotImplementedError):
        PK.cum_val([1.0, 2.0], 1.5, niter_max=20)
