"""CPU: chromosome selection by candidate spots without a device.  tests/harness/select_ref.py (the NumPy / SciPy statement
of segmentation_tools/chromosome.py:363-406 and spot_tools/picking.py:767-794) reproduces the reference's own outputs
(tests/golden/select.npz, written by scripts/make_select_golden.py), its incremental form equals its literal loop, the
rules csrc/select.hip relies on are pinned against the installed NumPy and SciPy, the public names have the reference's
signatures, and every argument error and early return comes before the device is touched."""
import ast
import inspect
import os
import re

import numpy as np
import pytest
from scipy.spatial.distance import cdist

import ref_loader
from conftest import load_golden
from harness import select_cases as K
from harness import select_ref as R

E = inspect.Parameter.empty
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold():
    return load_golden("select.npz")


@pytest.fixture(scope="module")
def records():
    """name -> (case, record of the incremental form), made once"""
    out = {}
    for name in K.CASES:
        c = K.case(name)
        out[name] = (c, R.incremental(*c))
    return out


def test_statement_reproduces_the_reference_outputs(gold, records):
    assert str(gold["source"]) == "reference"
    for name, (c, rec) in records.items():
        assert rec["raised"] == bool(gold[name + "_raised"]) == (name in K.RAISES), name
        assert rec["text"] == str(gold[name + "_text"]), name
        if not rec["raised"]:
            want = gold[name + "_kept"]
            assert rec["coords"].dtype == want.dtype and rec["coords"].shape == want.shape, name
            assert rec["coords"].tobytes() == want.tobytes(), name
        cands, spots_list, int_th, _ = c
        sel = R.selected(spots_list, int_th)[0][0]
        ids = [sel[rows, 4].astype(np.int64) for rows in R.assign(sel, cands)]
        assert np.array_equal(np.array([len(i) for i in ids]), gold[name + "_assign_counts"]), name
        assert np.array_equal(np.concatenate(ids), gold[name + "_assign_ids"]), name


def test_incremental_form_equals_the_literal_loop(records):
    """The literal loop stops without another pass once the flags it holds are at or below the threshold, so its ``lost``
    of the kept candidates dates from before the last removal; the incremental ``lost`` and owners are those of the final
    list, checked here against a fresh assignment to the kept candidates."""
    for name, (c, inc) in records.items():
        cands, spots_list, int_th, loss_th = c
        if name not in K.LITERAL_SLOW:
            lit = R.literal(*c)
            for k in ("kept", "removed", "removed_lost"):
                assert np.array_equal(inc[k], lit[k]), (name, k)
            assert inc["raised"] == lit["raised"] and inc["text"] == lit["text"], name
            assert inc["coords"].tobytes() == lit["coords"].tobytes(), name
            assert inc["visits"] <= lit["visits"], name
        if inc["raised"]:
            continue
        sels, _, starts = R.selected(spots_list, int_th)
        lost = np.zeros(len(inc["kept"]), dtype=np.int64)
        for r, sel in enumerate(sels):
            rows = R.assign(sel, inc["coords"])
            own = np.full(len(sel), -1, dtype=np.int64)
            for i, rr in enumerate(rows):
                lost[i] += len(rr) == 0
                own[rr] = inc["kept"][i]
            assert np.array_equal(own, inc["owner"][starts[r]:starts[r + 1]]), (name, r)
        assert np.array_equal(lost, inc["lost"][inc["kept"]]), name


def test_cases_hold_what_they_are_for(records):
    names = set(K.CASES)
    assert {len(records[n][0][0]) for n in names} >= {1, 2, 63, 64, 65, K.TILE - 1, K.TILE, K.TILE + 1, 2 * K.TILE + 37}
    sizes = {n: int(R.selected(records[n][0][1], records[n][0][2])[2][-1]) for n in names}
    assert {sizes["s0"], sizes["s1"], sizes["wg_less"], sizes["wg"], sizes["wg_more"]} == {0, 1, K.THREADS - 1, K.THREADS,
                                                                                          K.THREADS + 1}
    assert 19000 <= sizes["big"] <= 21000
    assert len(records["s1"][0][1]) == 1 and len(records["r40"][0][1]) == 40
    assert len(records["s1"][1]["kept"]) == 1 and len(records["s1"][1]["removed"]) == 2
    assert records["s0"][1]["raised"] and records["s0"][1]["removed"].tolist() == [0, 1, 2]
    assert isinstance(records["cand_list"][0][0], list) and records["float32"][0][1][0].dtype == np.float32
    for n in ("c63", "big", "tile_more", "chain", "r40"):
        assert len(records[n][1]["removed"]) >= 2, n
    # the chain: W goes first, then Y, whose spots take X from 6 lost rounds to 3
    rec = records["chain"][1]
    assert rec["removed"].tolist() == [3, 1] and rec["removed_lost"].tolist() == [10, 7] and rec["lost"].tolist() == [3, 7, 0, 10]
    # a removed duplicate never owned a spot: lost in every round
    cands = np.asarray(records["c63"][0][0])
    assert (cands[-1] == cands[:-2]).all(axis=1).any() and records["c63"][1]["lost"][-1] == 5
    # rounds without a selected spot among rounds with some: first, two in a row in the middle, last; some go, some stay
    per_round = np.diff(R.selected(records["gaps"][0][1], 0.5)[2])
    assert (per_round == 0).nonzero()[0].tolist() == [0, 3, 4, 13] and (per_round > 0).sum() == 10
    assert len(records["gaps"][0][1][0]) == 0 and len(records["gaps"][0][1][3]) > 0 and np.isnan(records["gaps"][0][1][4][:, 0]).all()
    rec = records["gaps"][1]
    assert len(rec["removed"]) >= 2 and len(rec["kept"]) >= 2 and rec["lost"].min() >= 4
    # odd values in selected rows
    _, zxys, _ = R.selected(records["odd_values"][0][1], 0.5)
    assert np.isnan(zxys).any() and np.isposinf(zxys).any() and np.isneginf(zxys).any()


def test_the_lattice_cases_contain_both_kinds_of_tie(records):
    exact, _ = R.tie_counts(*records["c63"][0][:3])
    assert exact > 0
    _, roots = R.tie_counts(*records["equal_roots"][0][:3])
    assert roots == 6            # every spot: the winner's sum is not the smallest, its root is
    rec = records["equal_roots"][1]
    assert rec["kept"].tolist() == [0] and rec["removed"].tolist() == [1, 2]


def test_cdist_is_the_stated_sum_of_squares():
    rs = np.random.RandomState(5)
    a, b = rs.rand(400, 3) * 3000, rs.rand(300, 3) * 3000
    d = a[:, None, :] - b[None, :, :]
    z2, x2, y2 = d[..., 0] * d[..., 0], d[..., 1] * d[..., 1], d[..., 2] * d[..., 2]
    want = cdist(a, b)
    assert np.sqrt((z2 + x2) + y2).tobytes() == want.tobytes()
    other = np.sqrt(z2 + (x2 + y2))
    assert (other != want).mean() > 0.02          # the association is really tested
    # float32 inputs are widened first
    a32, b32 = a.astype(np.float32), b.astype(np.float32)
    assert cdist(a32, b32).tobytes() == cdist(a32.astype(np.float64), b32.astype(np.float64)).tobytes()
    # the lattice data of the tests
    cands, spots_list, int_th, _ = K.case("c65")
    chrom = np.array(cands) * np.array(R.DISTANCE_ZXY)
    _, zxys, _ = R.selected(spots_list, int_th)
    d = zxys[:, None, :] - chrom[None, :, :]
    assert np.sqrt((d[..., 0] ** 2 + d[..., 1] ** 2) + d[..., 2] ** 2).tobytes() == cdist(zxys, chrom).tobytes()


def test_argmin_rules():
    nan, inf = np.nan, np.inf
    assert np.argmin([3.0, nan, 1.0, nan]) == 1              # the first NaN
    assert np.argmin([2.0, 1.0, 1.0]) == 1                   # the first minimum
    assert np.argmin([inf, inf]) == 0
    assert np.argmin(np.array([[5.0, 2.0, nan], [1.0, 1.0, 0.5]]), axis=1).tolist() == [2, 2]
    s = np.float64(3e17)
    while np.sqrt(np.nextafter(s, 0)) != np.sqrt(s):         # about every second pair of neighbours shares its root
        s = np.nextafter(s, np.inf)
    t = np.nextafter(s, 0)
    assert t < s and np.argmin(np.sqrt([s, t])) == 0         # decided by the roots, not by the sums
    # inf - inf is NaN, inf - finite is inf
    assert np.argmin(cdist([[inf, 0, 0]], [[0, 0, 0], [inf, 0, 0], [1, 1, 1]])[0]) == 1


def test_mean_of_bools_is_lost_over_rounds():
    for R_ in (1, 3, 7, 10, 40, 60, 333):
        for lost in range(R_ + 1):
            flags = [True] * lost + [False] * (R_ - lost)
            m = np.mean(flags)
            assert isinstance(m, np.float64) and m == np.float64(lost) / R_
            assert f"{m:.3f}" == f"{np.float64(lost) / R_:.3f}"
    with np.errstate(all="ignore"), pytest.warns(RuntimeWarning):
        assert np.isnan(np.mean([])) and not np.mean([]) > 0.4


SIGNATURES = {
    ("spot_tools.picking", "assign_spots_to_chromosomes"): [("spots", E), ("chrom_coords", E), ("distance_zxy", [200, 108, 108]),
                                                            ("dist_norm", 2)],
    ("segmentation_tools.chromosome", "select_candidate_chromosomes"): [("_cand_chrom_coords", E), ("_spots_list", E),
                                                                        ("_cand_spot_intensity_th", 0.5),
                                                                        ("_good_chr_loss_th", 0.4), ("_verbose", True)],
    ("classes.field_of_view", "select_chromosome_by_candidate_spots"): [("spots_list", E), ("cand_chrom_coords", E),
                                                                        ("_good_chr_loss_th", 0.4),
                                                                        ("_cand_spot_intensity_th", 0.5), ("_verbose", True),
                                                                        ("return_info", False)],
}


def test_names_and_signatures():
    import importlib
    for (mod, name), want in SIGNATURES.items():
        f = getattr(importlib.import_module("imageanalysis3_amd." + mod), name)
        got = [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
        assert got == want, (name, got)
    from imageanalysis3_amd.segmentation_tools import chromosome as CH
    assert issubclass(CH.NoChromosomeLeft, ValueError) and issubclass(CH.NoChromosomeLeft, NotImplementedError)
    from imageanalysis3_amd import _lib
    assert (_lib.SELECT_THREADS, _lib.SELECT_TILE) == (K.THREADS, K.TILE)


@pytest.mark.skipif(not ref_loader.available(), reason="reference tree not present")
def test_signatures_equal_the_reference_source():
    import importlib
    for path, mod, name in (("spot_tools/picking.py", "spot_tools.picking", "assign_spots_to_chromosomes"),
                            ("segmentation_tools/chromosome.py", "segmentation_tools.chromosome",
                             "select_candidate_chromosomes")):
        tree = ast.parse(open(os.path.join(ref_loader.REF, path)).read())
        fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == name][0]
        ref_names = [a.arg for a in fn.args.args]
        ref_defaults = [ast.unparse(d) for d in fn.args.defaults]
        f = getattr(importlib.import_module("imageanalysis3_amd." + mod), name)
        ps = list(inspect.signature(f).parameters.values())
        assert [p.name for p in ps] == ref_names
        ours = [p.default for p in ps if p.default is not E]
        assert len(ours) == len(ref_defaults)
        for o, r in zip(ours, ref_defaults):
            assert r == "_distance_zxy" and o == [200, 108, 108] or ast.literal_eval(r) == o, (name, o, r)


def test_ctypes_mirrors_match_the_header():
    from imageanalysis3_amd import _lib
    src = open(os.path.join(ROOT, "include", "ia3.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _lib.lib()
    for name in ("ia3_assign_nearest_dev", "ia3_select_chromosomes_dev"):      # prototypes and arity: test_abi_cpu.py
        assert re.search(r"\b%s\s*\(" % name, src) and name in _lib.EXPORTS and hasattr(lib, name)
    for define, value in (("IA3_SELECT_THREADS", _lib.SELECT_THREADS), ("IA3_SELECT_TILE", _lib.SELECT_TILE),
                          ("IA3_SELECT_EMPTY", _lib.IA3_SELECT_EMPTY)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % define, src).group(1)) == value


def test_argument_errors_and_early_returns_before_the_device(monkeypatch, capsys):
    from imageanalysis3_amd import _lib
    from imageanalysis3_amd.classes import field_of_view as F
    from imageanalysis3_amd.segmentation_tools import chromosome as CH
    from imageanalysis3_amd.spot_tools import picking as P

    def no_device(*a, **k):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(_lib, "lib", no_device)
    cands, spots_list, int_th, loss_th = K.case("c2")
    # no candidate: the reference's max() of an empty list
    for empty in ([], np.array([]), np.zeros((0, 3))):
        with pytest.raises(ValueError, match=r"^max\(\) arg is an empty sequence") as e:
            CH.select_candidate_chromosomes(empty, spots_list)
        assert isinstance(e.value, NotImplementedError) and "spot_tools.picking.assign_spots_to_chromosomes" in str(e.value)
        with pytest.raises(CH.NoChromosomeLeft):
            F.select_chromosome_by_candidate_spots(spots_list, empty, _verbose=False)
    assert capsys.readouterr().out.startswith("- start select from 0 chromosomes with loss threshold=0.4\n")
    # thresholds of 1 and above, NaN, and no rounds: every candidate, in the candidates' dtype
    for th in (1, 1.0, 2.5, np.inf, np.nan):
        out = CH.select_candidate_chromosomes(cands, spots_list, _good_chr_loss_th=th, _verbose=False)
        assert out.dtype == np.float64 and out.tobytes() == np.array(list(cands)).tobytes() and out is not cands
    out = CH.select_candidate_chromosomes(cands.astype(np.int32), [], _verbose=True)
    assert out.dtype == np.int32 and np.array_equal(out, cands)
    assert capsys.readouterr().out == ("- start select from 2 chromosomes with loss threshold=0.4\n"
                                       "-- 2 chromosomes are kept.\n")
    got = F.select_chromosome_by_candidate_spots([], cands, _verbose=False, return_info=True)
    assert np.array_equal(got[0], cands) and len(got[1]) == 0 and got[2] is None and got[3] is None
    # malformed tables fail as NumPy / cdist fail them
    with pytest.raises(IndexError):
        CH.select_candidate_chromosomes(cands, [[]], _verbose=False)                    # np.array([])[:, 0]
    with pytest.raises(IndexError):
        CH.select_candidate_chromosomes(cands, [np.arange(5.0)], _verbose=False)
    with pytest.raises(ValueError):
        CH.select_candidate_chromosomes(cands, [spots_list[0][:, :3]], _verbose=False)   # two coordinate columns
    with pytest.raises(ValueError):
        CH.select_candidate_chromosomes(cands[:, :2], spots_list, _verbose=False)        # cannot broadcast with distance_zxy
    with pytest.raises(ValueError):
        CH.select_candidate_chromosomes([1.0, 2.0, 3.0], spots_list, _verbose=False)     # XB must be 2-dimensional
    # the untouched device is really what the valid call reaches
    with pytest.raises(AssertionError, match="device"):
        CH.select_candidate_chromosomes(cands, spots_list, _verbose=False)
    # assign_spots_to_chromosomes
    assert P.assign_spots_to_chromosomes([], cands) == [[], []]
    assert P.assign_spots_to_chromosomes(np.zeros((0, 5)), cands) == [[], []]
    with pytest.raises(ValueError):
        P.assign_spots_to_chromosomes(spots_list[0], cands[:, :2])
    with pytest.raises(ValueError, match="argmin"):
        P.assign_spots_to_chromosomes(spots_list[0], np.zeros((0, 3)))
    with pytest.raises(ValueError):
        P.assign_spots_to_chromosomes(spots_list[0][:, :3], cands)
    with pytest.raises(AssertionError, match="device"):
        P.assign_spots_to_chromosomes(spots_list[0], cands)
    for bad in (np.zeros((4, 2)), np.zeros(3)):
        with pytest.raises(ValueError):
            _lib.assign_nearest(bad, cands)
    with pytest.raises(ValueError, match="round_start"):
        _lib.select_chromosomes(np.zeros((4, 3)), [0, 3], cands, 0.4)
