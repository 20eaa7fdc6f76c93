"""GPU: the compartment densities on the device (csrc/density.hip) against the reference's own outputs
(tests/golden/compartment_density.npz) through the reference-named functions, the flat form on a resident population and
the C entries.

The argument of exp is NumPy's bit for bit, exp is the device library's, and a sum is made of partial sums over 64
consecutive contributors added in order, so with every term >= 0 the relative error of a sum of n terms is at
most 2 * 2**-52 + (64 + n / 64 + 2) * 2**-53 < 1.3e-13 for n <= 65 536.  The tests allow 1e-12 relative, 8 x that bound, plus
2.3e-308 per row for terms in the subnormal range that come out flushed or not.  NaN positions and the counts of rows are
exact.  The first test prints the largest relative error it saw; on an MI355X it was 7.7e-16."""
import numpy as np
import pytest

from conftest import load_golden
from harness import density_cases as K

pytestmark = pytest.mark.gpu

RTOL, TINY = 1e-12, 2.3e-308


@pytest.fixture(scope="module")
def L():
    from imageanalysis3_amd import _lib
    _lib.check(_lib.lib().ia3_init(0))
    return _lib


@pytest.fixture(scope="module")
def D(L):
    from imageanalysis3_amd.compartment_tools import density
    return density


@pytest.fixture(scope="module")
def gold():
    return load_golden("compartment_density.npz")


@pytest.fixture(scope="module")
def cells():
    return K.cells()


@pytest.fixture(scope="module")
def pop(L, cells):
    """Every cell of the cases in one resident population."""
    with L.DensityPopulation.upload(cells, K.AB) as p:
        yield p


def columns(pop, indices):
    """The points of the given cells in the population's order."""
    s = pop.layout.cell_start
    return np.concatenate([np.arange(s[i], s[i + 1]) for i in indices])


worst = {"rel": 0.0}


def close(got, ref, count):
    """|got - ref| <= 1e-12 |ref| + count * 2.3e-308, a NaN for a NaN; notes the largest relative error."""
    assert got.shape == ref.shape and got.dtype == np.float64
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    ok = ~np.isnan(ref)
    err = np.abs(got[ok] - ref[ok])
    big = ref[ok] > 1e-290
    if big.any():
        worst["rel"] = max(worst["rel"], float((err[big] / ref[ok][big]).max()))
    return bool((err <= RTOL * np.abs(ref[ok]) + np.maximum(count[ok], 0) * TINY).all())


@pytest.mark.parametrize("tag", ["small", "large"])
def test_resident_population_equals_the_reference(L, D, gold, pop, tag):
    """All sixteen totals, the NaN cell and the far cell in one call per option set; the labels and sigmas change, the
    coordinates stay where they are."""
    indices, options = (K.small_indices(), K.full_options()) if tag == "small" else (K.large_indices(), K.LARGE_OPTIONS)
    cols = columns(pop, indices)
    for c, t, x, n, s in options:
        got, cnt = D.population_compartment_densities(pop, K.AB, K.SIGMAS[s], normalize_by_reg_num=bool(n), exclude_self=bool(x),
                                                      use_cis=bool(c), use_trans=bool(t), return_counts=True)
        assert got.shape == (2, pop.n_points) and cnt.dtype == np.int32
        ref, ref_cnt = gold["%s_%s" % (tag, K.option_name(c, t, x, n, s))], gold["%scnt_c%dt%dx%d" % (tag, c, t, x)]
        counted = ref_cnt >= 0          # where the reference gives NaN before any row is added, nothing is counted by it
        assert np.array_equal(cnt[:, cols][counted], ref_cnt[counted]), (tag, c, t, x)
        assert close(got[:, cols], ref, ref_cnt), (tag, c, t, x, n, s)
    print("largest relative error so far: %.3e" % worst["rel"])
    assert worst["rel"] < RTOL


def test_reference_named_functions(D, gold, cells):
    """BatchCompartmentDensities with its own defaults (normalised), and the single-cell function with its (not)."""
    idx = K.small_indices()
    out = D.BatchCompartmentDensities([cells[i] for i in idx], K.AB, K.SIGMAS["scalar"], num_threads=3)
    assert isinstance(out, list) and len(out) == len(idx)
    for i, o in zip(idx, out):
        assert list(o) == list(cells[i])
        assert all(list(o[c]) == ['A', 'B'] and o[c]['A'].shape == cells[i][c].shape[:2] and o[c]['B'].dtype == np.float64 for c in o)
    cnt = gold["smallcnt_c0t1x1"]
    assert close(K.flat(out), gold["small_" + K.option_name(0, 1, 1, 1, "scalar")], cnt)
    one = [D.calculate_compartment_densities(cells[i], K.AB, K.SIGMAS["scalar"]) for i in idx]
    assert close(K.flat(one), gold["small_" + K.option_name(0, 1, 1, 0, "scalar")], cnt)
    both = [D.calculate_compartment_densities(cells[i], K.AB, K.SIGMAS["aniso"], True, False, True, True) for i in idx]
    assert close(K.flat(both), gold["small_" + K.option_name(1, 1, 0, 1, "aniso")], gold["smallcnt_c1t1x0"])
    # the cells of one copy: NaN for trans alone, the cis sum otherwise
    assert np.isnan(one[0]['a']['A']).all() and np.isnan(one[1]['b']['B']).all()
    # (region 0 of 'b' and the one region of 'a' are their own only A row: exp(0) / 1; 'a' lists nothing under B: 0 / 0)
    assert both[1]['b']['A'][0, 0] == 1.0 and np.isnan(both[0]['a']['B']).all() and both[0]['a']['A'].tolist() == [[1.0]]


def test_each_cell_alone_equals_the_batch_and_runs_repeat(L, D, pop, cells):
    """Bit for bit: a cell's result does not depend on the other cells of the call, and two runs agree."""
    for opt in ((0, 1, 1, 0, "scalar"), (1, 1, 0, 0, "aniso")):
        c, t, x, n, s = opt
        kw = dict(normalize_by_reg_num=bool(n), exclude_self=bool(x), use_cis=bool(c), use_trans=bool(t), return_counts=True)
        batch, bcnt = D.population_compartment_densities(pop, K.AB, K.SIGMAS[s], **kw)
        again, acnt = D.population_compartment_densities(pop, K.AB, K.SIGMAS[s], **kw)
        assert batch.tobytes() == again.tobytes() and bcnt.tobytes() == acnt.tobytes()
        start = pop.layout.cell_start
        for i, cell in enumerate(cells):
            with L.DensityPopulation.upload([cell], K.AB) as alone:
                got, cnt = D.population_compartment_densities(alone, K.AB, K.SIGMAS[s], **kw)
            assert got.tobytes() == batch[:, start[i]:start[i + 1]].tobytes(), (opt, i)
            assert cnt.tobytes() == bcnt[:, start[i]:start[i + 1]].tobytes(), (opt, i)


def test_new_labels_on_the_resident_population_equal_a_fresh_upload(L, D, pop, cells):
    rs = np.random.RandomState(5)
    shuffled = {}
    for c, R in K.REGIONS.items():       # randomize_index_dict's effect: other regions under the same keys
        p = rs.permutation(R)
        shuffled[c] = {'A': p[:R // 2], 'B': p[R // 2:]}
    before = D.population_compartment_densities(pop, K.AB, 300.0)
    moved = D.population_compartment_densities(pop, shuffled, [200.0, 350.0, 300.0], use_cis=True)
    with L.DensityPopulation.upload(cells, shuffled) as fresh:
        want = D.population_compartment_densities(fresh, shuffled, [200.0, 350.0, 300.0], use_cis=True)
    assert moved.tobytes() == want.tobytes() and moved.tobytes() != before.tobytes()
    assert D.population_compartment_densities(pop, K.AB, 300.0).tobytes() == before.tobytes()


def test_gaussian_density_terms(D, gold):
    centers, ref, triples = K.gaussian_case()
    for i, (sigma, intensity, background) in enumerate(triples):
        got = D.calculate_gaussian_density(centers, ref, sigma, intensity, background)
        want = gold["gauss_%d" % i]
        assert got.shape == want.shape == (70,) and np.array_equal(np.isnan(got), np.isnan(want))
        ok = ~np.isnan(want)
        # intensity * g + background in float64 on the host: the term's two ulps, then one rounding each
        assert (np.abs(got[ok] - want[ok]) <= RTOL * np.abs(want[ok]) + TINY).all()
    assert got[9] == -1.0 and np.isnan(got[5])
    block = D.calculate_gaussian_density(centers.reshape(7, 10, 3), ref, 300.0)
    assert block.shape == (7, 10) and block.ravel().tobytes() == D.calculate_gaussian_density(centers, ref, 300.0).tobytes()
    single = D.calculate_gaussian_density(centers[3], ref, 300.0)
    assert np.ndim(single) == 0 and single == block[0, 3]


def test_library_argument_errors(L):
    import ctypes as C
    zxys = np.zeros((5, 3))
    copy_of, locus_of = np.array([0, 0, 1, 0, 0], dtype=np.int32), np.array([0, 1, 0, 0, 1], dtype=np.int32)
    start = np.array([0, 3, 5], dtype=np.int32)

    def create(zxys=zxys, start=start, copy_of=copy_of, locus_of=locus_of, n_cells=2, n_loci=2, out=True):
        h = C.c_void_p()
        rc = L.lib().ia3_density_create(None if zxys is None else L.ptr(zxys), None if start is None else L.ptr(start),
                                        None if copy_of is None else L.ptr(copy_of), None if locus_of is None else L.ptr(locus_of),
                                        n_cells, n_loci, C.byref(h) if out else None)
        if rc == L.IA3_OK:
            L.lib().ia3_density_free(h)
        else:
            assert not h.value
        return rc

    assert create() == L.IA3_OK
    for kw in (dict(zxys=None), dict(start=None), dict(copy_of=None), dict(locus_of=None), dict(out=False), dict(n_cells=0),
               dict(n_loci=0), dict(start=np.array([1, 3, 5], dtype=np.int32)), dict(start=np.array([0, 4, 3], dtype=np.int32)),
               dict(locus_of=np.array([0, 2, 0, 0, 1], dtype=np.int32)), dict(locus_of=np.array([0, -1, 0, 0, 1], dtype=np.int32)),
               dict(copy_of=np.array([0, -1, 1, 0, 0], dtype=np.int32)), dict(copy_of=np.array([0, 65536, 1, 0, 0], dtype=np.int32)),
               dict(start=np.array([0, 65537], dtype=np.int32), n_cells=1)):
        assert create(**kw) == L.IA3_EINVAL, list(kw)
    with L.DensityPopulation.upload([{'1': np.zeros((2, 2, 3))}], ['1']) as p:
        mult, s2 = np.ones((2, 2), dtype=np.uint8), np.ones(3)
        sums, counts = np.zeros((2, 4)), np.zeros((2, 4), dtype=np.int32)

        def rc(h=p._h, mult=mult, s2=s2, cis=0, trans=1, sums=sums, counts=counts):
            return L.lib().ia3_density_scores_dev(h, None if mult is None else L.ptr(mult), None if s2 is None else L.ptr(s2), cis,
                                                  trans, 1, None if sums is None else L.ptr(sums), None if counts is None else L.ptr(counts))

        assert rc() == L.IA3_OK and counts.tolist() == [[2] * 4] * 2 and sums.tolist() == [[2.0] * 4] * 2
        for kw in (dict(h=None), dict(mult=None), dict(s2=None), dict(sums=None), dict(counts=None), dict(cis=0, trans=0)):
            assert rc(**kw) == L.IA3_EINVAL, list(kw)
        with pytest.raises(ValueError):
            p.scores(np.ones((3, 2), dtype=np.uint8), s2)
        with pytest.raises(ValueError):
            p.scores(mult, np.ones(2))
    # a cell of the cap's size is taken (one workgroup row of queries is enough to see it run)
    big = np.zeros((1, L.IA3_DENSITY_MAX_CELL, 3))
    with L.DensityPopulation.upload([{'1': big}], ['1']) as p:
        assert p.n_points == L.IA3_DENSITY_MAX_CELL
