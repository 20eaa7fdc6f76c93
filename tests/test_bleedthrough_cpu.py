"""CPU: the host side of the bleedthrough-profile generator (correction_tools/bleedthrough.py) against what the
reference's own functions returned (tests/golden/bleedthrough.npz / .json, scripts/make_bleedthrough_golden.py): names
and signatures, check_bleedthrough_info, check_bleedthrough_pairs, and the polynomial constants fitted to the
reference's own pairs."""
import json
import os

import numpy as np
import pytest

from conftest import load_golden
from harness import bleed_ref as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return load_golden("bleedthrough.npz")


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(ROOT, "tests", "golden", "bleedthrough.json")) as f:
        return json.load(f)


def test_names_signatures_and_defaults(recorded):
    from imageanalysis3_amd.correction_tools import bleedthrough as bl
    for name, sig in recorded["signatures"].items():
        assert B.signature_record(getattr(bl, name)) == sig, name
    assert bl._bleedthrough_channels == recorded["defaults"]["_bleedthrough_channels"]
    assert sorted(bl._bleedthrough_default_correction_args) == recorded["defaults"]["_bleedthrough_default_correction_args"]
    assert bl._bleedthrough_default_fitting_args == recorded["defaults"]["_bleedthrough_default_fitting_args"]
    assert callable(bl._bleedthrough_constants) and callable(bl.bleedthrough_profile_from_pairs)


def test_abi_symbol_exported():
    from imageanalysis3_amd import _lib
    assert "ia3_bleedthrough_profile_dev" in _lib.EXPORTS and hasattr(_lib.lib(), "ia3_bleedthrough_profile_dev")
    assert "ia3_bleedthrough_profile_dev" in open(os.path.join(ROOT, "include", "ia3.h")).read()


def test_check_bleedthrough_info_decisions(recorded):
    from imageanalysis3_amd.correction_tools.bleedthrough import check_bleedthrough_info
    cases = B.info_cases()
    assert sorted(recorded["check_info"]) == sorted(c[0] for c in cases)
    for name, info, kw in cases:
        got = check_bleedthrough_info(info, **kw)
        assert got is recorded["check_info"][name], name


@pytest.mark.parametrize("tag,kw", B.PAIR_CASES)
def test_check_bleedthrough_pairs_keeps_the_reference_set(golden, recorded, tag, kw):
    from imageanalysis3_amd.correction_tools.bleedthrough import check_bleedthrough_pairs
    infos = B.pair_infos()
    kept = check_bleedthrough_pairs(infos, verbose=False, **kw)
    assert np.array_equal([i['id'] for i in kept], golden["pairs_kept_" + tag])
    assert all(k is infos[k['id']] for k in kept)                # the infos themselves, in order
    assert recorded["conditions"]["b_min_relative_margin"] > 1e-9


def test_delaunay_neighbours_equal_the_scan():
    from scipy.spatial import Delaunay
    from imageanalysis3_amd.correction_tools.bleedthrough import _delaunay_neighbors
    coords = np.array([i['coord'] for i in B.pair_infos()])
    pts = np.concatenate([coords[:40], coords[:1] + 200.0])
    tri = Delaunay(pts)
    got = _delaunay_neighbors(tri.simplices, len(pts))
    for i in range(len(pts)):
        assert np.array_equal(got[i], np.unique(np.array([s for s in tri.simplices if i in s], dtype=int))), i
    assert all(len(g) == 0 for g in _delaunay_neighbors(np.zeros((0, 4), dtype=int), 3))


def _golden_info_dicts(golden):
    """The reference's pairs of every used movie, as find_bleedthrough_pairs returned them (boxes left out: the checks
    that read them were made when the fixture was written, their results are pairs_*_kept)."""
    dicts = []
    for name in B.USED_NAMES:
        for c in B.CHANNELS:
            d = {}
            for t in B.CHANNELS:
                if t == c:
                    continue
                pre = "pairs_%d_%s_to_%s_" % (B.movie_number(name), c, t)
                keep = golden[pre + "kept"]
                d["%s_to_%s" % (c, t)] = [
                    {'coord': golden[pre + "coord"][i], 'spot': golden[pre + "spot"][i], 'rsquare': float(golden[pre + "rsquare"][i]),
                     'slope': golden[pre + "slope"][i], 'intercept': golden[pre + "intercept"][i]}
                    for i in range(len(keep)) if keep[i]]
            dicts.append(d)
    return dicts


@pytest.mark.parametrize("tag,order", [("o2_2d", 2), ("o1_2d", 1)])
def test_constants_of_the_reference_pairs(golden, tag, order):
    """_bleedthrough_constants on the reference's pairs: the pairs its outlier check kept, and its constants to the
    reproducibility of scipy.linalg.lstsq (1e-9 relative to the largest constant's design column scale: the same LAPACK
    driver on the same matrix, allowing for another build of it)."""
    from imageanalysis3_amd.correction_tools import bleedthrough as bl
    dicts = _golden_info_dicts(golden)
    k, seen = 0, []
    real = bl.check_bleedthrough_pairs

    def watching(info_list, **kw):
        out = real(info_list, **kw)
        ids = {id(i) for i in out}
        seen.append(np.array([id(i) in ids for i in info_list]))
        return out
    bl.check_bleedthrough_pairs = watching
    try:
        for r in B.CHANNELS:
            for t in B.CHANNELS:
                if r == t:
                    continue
                fit = bl._bleedthrough_constants(dicts, r, t, min_num_spots=B.MIN_NUM_SPOTS, fitting_order=order, verbose=False)
                if B.SLOPES[(r, t)] is None:
                    assert fit is None
                    continue
                for got, want in ((fit[0], golden["gen_%s_C_slope" % tag][k]), (fit[1], golden["gen_%s_C_intercept" % tag][k])):
                    assert got.shape == want.shape == (bl.L.poly_columns(order),)
                    assert np.all(np.abs(got - want) <= 1e-9 * np.abs(want).max()), (r, t)
                assert 0.0 < fit[2] <= 1.0 and fit[3] <= 1.0
                k += 1
    finally:
        bl.check_bleedthrough_pairs = real
    assert k == 5 and np.array_equal(np.concatenate(seen), golden["gen_%s_checked" % tag])


def test_zero_profile_and_argument_errors(golden):
    from imageanalysis3_amd.correction_tools import bleedthrough as bl
    assert bl._bleedthrough_constants([{}], '750', '647', verbose=False) is None
    s, i = bl.interploate_bleedthrough_correction_from_channel([], '750', '647', single_im_size=[2, 3, 4], verbose=False)
    assert s.shape == (2, 3, 4) and s.dtype == np.float64 and not s.any() and not i.any()
    with pytest.raises(ValueError):
        bl.find_bleedthrough_pairs("x.dax", '488')
    with pytest.raises(NotImplementedError):
        bl._profile_arguments([], B.CHANNELS, 4, {})
    with pytest.raises(TypeError):
        bl._profile_arguments([], B.CHANNELS, 2, {'fitting_order': 1})
