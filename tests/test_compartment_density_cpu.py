"""No GPU: the reference's names and signatures of compartment_tools/density.py, the argument errors that come before any
device call, the packing of cells into copies, locus ids and multiplicities, the fixture (tests/golden/
compartment_density.npz, the reference's own outputs) against the cases, the ctypes mirrors against include/ia3.h, and the
stand-alone check of csrc/ia3_density.h (tests/native/density_cpu.cpp), also under AddressSanitizer and UBSan."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import load_golden
from harness import density_cases as K

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def gold():
    return load_golden("compartment_density.npz")


@pytest.fixture(scope="module")
def D():
    from imageanalysis3_amd.compartment_tools import density
    return density


def test_names_and_signatures_are_the_references(D, gold):
    for name in ("calculate_gaussian_density", "calculate_compartment_densities", "BatchCompartmentDensities"):
        assert str(inspect.signature(getattr(D, name))) == str(gold["sig_" + name]), name
    assert str(inspect.signature(D.population_compartment_densities)) == \
        "(population, chr_2_AB_dict, gaussian_radius, normalize_by_reg_num=False, exclude_self=True, use_cis=False, " \
        "use_trans=True, return_counts=False)"
    assert inspect.signature(D.BatchCompartmentDensities).parameters["normalize_by_reg_num"].default is True
    assert inspect.signature(D.calculate_compartment_densities).parameters["normalize_by_reg_num"].default is False


def test_scoring_and_calling_stay_absent():
    import imageanalysis3_amd.compartment_tools as ct
    assert hasattr(ct, "density")
    for name in ("scoring", "calling"):
        with pytest.raises(ImportError):
            __import__("imageanalysis3_amd.compartment_tools." + name)


def test_ctypes_mirrors_match_the_header():
    from imageanalysis3_amd import _lib
    src = open(os.path.join(ROOT, "include", "ia3.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    found = re.findall(r"\b(?:int|void)\s+(ia3_density_[a-z_]+)\s*\(", src)
    assert sorted(found) == sorted(e for e in _lib.EXPORTS if e.startswith("ia3_density_")) and len(found) == 3
    assert int(re.search(r"#define IA3_DENSITY_MAX_CELL (\d+)", src).group(1)) == _lib.IA3_DENSITY_MAX_CELL == 65536
    hdr = open(os.path.join(ROOT, "imageanalysis3_amd", "csrc", "ia3_density.h")).read()
    assert int(re.search(r"DN_CELL_MAX = (\d+)", hdr).group(1)) == _lib.IA3_DENSITY_MAX_CELL
    assert issubclass(_lib.DensityPopulation, _lib.Owner)
    assert "free" not in vars(_lib.DensityPopulation) and "__del__" not in vars(_lib.DensityPopulation)


def test_errors_come_before_any_device_call(D):
    """This test runs without a device: a call that reached the library would raise IA3Error instead."""
    cell = {'c': np.zeros((2, 7, 3)), 'b': np.ones((1, 2, 3))}
    for fn, arg in ((D.calculate_compartment_densities, cell), (D.BatchCompartmentDensities, [cell])):
        with pytest.raises(ValueError, match="One of use_cis or use_trans should be true!"):
            fn(arg, K.AB, 300.0, use_cis=False, use_trans=False)
        with pytest.raises(KeyError):
            fn(arg, {'c': K.AB['c']}, 300.0)
        with pytest.raises(KeyError):
            fn(arg, {'c': K.AB['c'], 'b': {'A': [0]}}, 300.0)
        with pytest.raises(ValueError):
            fn(arg, K.AB, [300.0, 200.0])
    with pytest.raises(ValueError, match="One of use_cis or use_trans should be true!"):
        D.population_compartment_densities(None, K.AB, 300.0, use_cis=False, use_trans=False)
    for bad in (np.zeros((0, 7, 3)), np.zeros((2, 0, 3)), np.zeros((2, 7, 2)), np.zeros((7, 3)), np.zeros((1, 65537, 3))):
        with pytest.raises(ValueError):
            D.calculate_compartment_densities({'c': bad}, K.AB, 300.0)
    for bad in ([7], [-1], [0, 1, 70], np.array([0.0, 1.0]), np.array([True] * 7)):
        with pytest.raises(IndexError):
            D.calculate_compartment_densities(cell, dict(K.AB, c={'A': bad, 'B': [1]}), 300.0)
        with pytest.raises(IndexError):
            D.calculate_compartment_densities(cell, dict(K.AB, c={'A': [1], 'B': bad}), 300.0, use_cis=True, use_trans=False)
    # an index that one cell allows and another does not
    with pytest.raises(IndexError):
        D.BatchCompartmentDensities([{'c': np.zeros((1, 7, 3))}, {'c': np.zeros((1, 4, 3))}], {'c': {'A': [5], 'B': []}}, 300.0)
    with pytest.raises(NotImplementedError):
        D.calculate_compartment_densities(cell, dict(K.AB, c={'A': [2] * 256, 'B': [1]}), 300.0)
    with pytest.raises(ValueError):
        D.calculate_gaussian_density(np.zeros((4, 2)), np.zeros(3), 1.0)
    with pytest.raises(ValueError):
        D.calculate_gaussian_density(np.zeros((4, 3)), np.zeros(2), 1.0)
    with pytest.raises(ValueError):
        D.calculate_gaussian_density(np.zeros((4, 3)), np.array([0.0, np.inf, 0.0]), 1.0)
    with pytest.raises(ValueError):
        D.calculate_gaussian_density(np.zeros((4, 3)), np.zeros(3), [1.0, 2.0])
    # a NaN reference needs no arithmetic: every term is NaN
    out = D.calculate_gaussian_density(np.zeros((2, 4, 3)), np.array([0.0, np.nan, 0.0]), 1.0, intensity=3, background=1)
    assert out.shape == (2, 4) and np.isnan(out).all()
    assert D.BatchCompartmentDensities([], K.AB, 300.0) == []


def test_packing_of_a_hand_written_cell():
    from imageanalysis3_amd import _lib
    z1 = np.arange(2 * 3 * 3, dtype=np.float64).reshape(2, 3, 3)
    z2 = 100.0 + np.arange(1 * 2 * 3, dtype=np.float64).reshape(1, 2, 3)
    z3 = 200.0 + np.arange(3 * 2 * 3, dtype=np.float64).reshape(3, 2, 3)
    cells = [{'1': z1, '2': z2}, {}, {'2': z3, '1': z1[:1, :2]}]
    labels = {'X': {'A': [0], 'B': []}, '1': {'A': [0, 0, 2], 'B': np.array([1])}, '2': {'A': [], 'B': (1, 1, 0)}}
    lay = _lib.DensityLayout(cells, labels)
    assert lay.chrs == ['X', '1', '2'] and lay.regions == {'X': 0, '1': 3, '2': 2} and lay.least_regions == {'1': 2, '2': 2}
    assert lay.first_id == {'X': 0, '1': 0, '2': 3} and lay.n_loci == 5 and lay.n_points == 16
    assert lay.cell_start.tolist() == [0, 8, 8, 16] and lay.cell_start.dtype == np.int32
    assert lay.n_copies.tolist() == [3, 0, 4]
    assert lay.copy_of.tolist() == [0, 0, 0, 1, 1, 1, 2, 2] + [0, 0, 1, 1, 2, 2, 3, 3]
    assert lay.locus_of.tolist() == [0, 1, 2, 0, 1, 2, 3, 4] + [3, 4, 3, 4, 3, 4, 0, 1]
    assert lay.zxys.shape == (16, 3) and lay.zxys.flags.c_contiguous
    assert np.array_equal(lay.zxys[:6], z1.reshape(-1, 3)) and np.array_equal(lay.zxys[8:14], z3.reshape(-1, 3))
    assert lay.blocks[2] == [('2', 3, 2, 8), ('1', 1, 2, 14)]
    with pytest.raises(IndexError):      # region 2 of '1' is outside the third cell's two regions
        lay.multiplicities(labels)
    labels['1']['A'] = [0, 0, 1]
    mult = lay.multiplicities(labels)
    assert mult.dtype == np.uint8 and mult.tolist() == [[2, 0], [1, 1], [0, 0], [0, 1], [0, 2]]
    out = lay.unpack(np.arange(32, dtype=np.float64).reshape(2, 16))
    assert [list(o) for o in out] == [['1', '2'], [], ['2', '1']]
    assert out[0]['1']['A'].tolist() == [[0, 1, 2], [3, 4, 5]] and out[2]['1']['B'].tolist() == [[30, 31]]
    assert out[2]['2']['A'].shape == (3, 2)
    with pytest.raises(KeyError):
        _lib.DensityLayout(cells, ['1'])


def test_cases_have_the_totals_and_the_edges():
    cells = K.cells()
    totals = [sum(z.shape[0] * z.shape[1] for z in c.values()) for c in cells]
    assert tuple(totals[:len(K.TOTALS)]) == K.TOTALS == (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 600, 1100)
    assert totals[-2:] == [33, 32]
    edge = cells[K.TOTALS.index(129)]
    pts = np.concatenate([z.reshape(-1, 3) for z in edge.values()])
    assert np.isnan(pts).any() and (np.isinf(pts) & ~np.isnan(pts)).any()
    assert any(z.shape[0] == 1 for z in edge.values()) and any(z.shape[0] > 1 for z in edge.values())
    assert all(np.isnan(z).all() for z in cells[-2].values())
    assert sum(z.shape[0] for z in cells[0].values()) == 1 and sum(z.shape[0] for z in cells[1].values()) == 1
    a, b = np.asarray(K.AB['c']['A']), np.asarray(K.AB['c']['B'])
    assert len(a) != len(np.unique(a)) and set(range(7)) - set(a) - set(b)
    far = cells[-1]['d']
    gap = (far[1, :, 1] - far[0, :, 1]) / K.SIGMA_X
    assert 36.9 < gap.min() < 37.2 and 39.3 < gap.max() < 39.6


def _expected_nan(cells, indices, use_cis):
    """NaN of the unnormalised sums: a query with a NaN coordinate, or trans alone in a cell of a single copy."""
    out = []
    for i in indices:
        single = sum(z.shape[0] for z in cells[i].values()) < 2
        for z in cells[i].values():
            out.append(np.isnan(z).any(axis=2).ravel() | (single and not use_cis))
    return np.concatenate(out)


def test_fixture_matches_the_cases(gold):
    cells = K.cells()
    assert str(gold["source"]) == "reference"
    for tag, indices, options in (("small", K.small_indices(), K.full_options()), ("large", K.large_indices(), K.LARGE_OPTIONS)):
        n = sum(z.shape[0] * z.shape[1] for i in indices for z in cells[i].values())
        for c, t, x, nrm, s in options:
            v = gold["%s_%s" % (tag, K.option_name(c, t, x, nrm, s))]
            cnt = gold["%scnt_c%dt%dx%d" % (tag, c, t, x)]
            assert v.shape == (2, n) and v.dtype == np.float64 and cnt.shape == (2, n) and cnt.dtype == np.int32
            nan = _expected_nan(cells, indices, c)
            assert np.array_equal(cnt < 0, np.stack([nan, nan]))
            assert np.array_equal(np.isnan(v), (cnt < 0) | ((cnt == 0) & bool(nrm)))
            assert (v[~np.isnan(v)] >= 0).all()
            if not nrm:     # the unnormalised sum of no row is 0.0, and a sum is at most its number of rows
                assert (v[cnt == 0] == 0).all() and (v[cnt > 0] <= cnt[cnt > 0]).all()
    v = gold["small_" + K.option_name(0, 1, 1, 0, "scalar")][:, -32:]
    assert (v == 0).any() and ((v > 0) & (v < 2.3e-308)).any() and (v > 2.3e-308).any()
    assert len(gold["arg_t"]) == len(K.arg_case()) and gold["gauss_0"].shape == (70,)
    assert np.isnan(gold["gauss_0"][5]) and gold["gauss_0"][9] == 0 and gold["gauss_1"][9] == 10


# ---- csrc/ia3_density.h on the host -----------------------------------------------------------------------------------------

SRC = os.path.join(HERE, "native", "density_cpu.cpp")
HDR = os.path.join(ROOT, "imageanalysis3_amd", "csrc", "ia3_density.h")
EXE = os.path.join(HERE, "native", "density_cpu")


def _build(exe, extra=()):
    if not os.path.isfile(exe) or os.path.getmtime(exe) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off"] + list(extra) + ["-o", exe, SRC])
    return exe


def _check(exe, gold, tmp_path):
    v = K.arg_case()
    rows = np.concatenate([v[:, :6], v[:, 6:]**2, gold["arg_t"][:, None]], axis=1)
    path = tmp_path / "args.f64"
    np.ascontiguousarray(rows, dtype=np.float64).tofile(str(path))
    p = subprocess.run([exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(p.stdout[-3000:])
    assert p.returncode == 0, p.stdout[-2000:]
    m = re.search(r"args (\d+) mismatches (\d+)", p.stdout)
    assert m and int(m.group(1)) == len(v) == 4096 and int(m.group(2)) == 0
    table = [tuple(int(x) for x in r) for r in re.findall(r"^w (\d) (\d) (\d) (\d) (\d)$", p.stdout, flags=re.M)]
    assert table == K.weight_table() and len(table) == 96
    m = re.search(r"pack (\d+) (\d+)", p.stdout)
    assert m and int(m.group(1)) == 80 and int(m.group(2)) == 0


def test_argument_and_weight_rule_on_the_host(gold, tmp_path):
    _check(_build(EXE), gold, tmp_path)


def test_argument_and_weight_rule_under_sanitizers(gold, tmp_path):
    """the same stand-alone program with AddressSanitizer and UBSan (a host program of its own: nothing is preloaded)"""
    _check(_build(EXE + "_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]), gold, tmp_path)
