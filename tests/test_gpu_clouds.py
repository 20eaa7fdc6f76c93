"""GPU: the Gaussian sources and the density clouds on the device (csrc/cloud.hip) against the reference's own outputs
(tests/golden/clouds.npz) through the reference-named functions, the flat batch form and the list form.

The box of a source and the argument of exp are NumPy's bit for bit; only exp differs, the device's and NumPy's each within
1 ulp of the true value, so a kernel value K differs by at most 2 * 2**-52 * K.  From that:

float64 sums.  A term h * K carries that difference and one rounding on either side, 3 * 2**-52 * |h| * K; each of the n
additions of a voxel rounds once on either side, 2**-53 of a partial sum that is at most |input| + S, S = sum |h_i| * K_i over
the sources that reach the voxel.  |got - ref| <= 3 * 2**-52 * S + n * 2**-52 * (|input| + S).  The bound is in S, not in the
result, because h may be negative.  The tests allow 8 x that, plus 2.3e-308 * sum |h_i| for kernel values in the subnormal
range that come out flushed or not.

float32 rounded after every source, all h >= 0.  The running value only grows; a source moves it by at most one float32 ulp
of the final value away from the reference's, so |got - ref| <= n * ulp32(ref).  The tests allow exactly that (no margin: it
already assumes that every source flips a rounding).  After a normalisation the same in relative terms, with two roundings
of the divisions and, for normalize_pdf, the perturbation of the sum (at most that of its largest term, all being >= 0):
|got - ref| <= (n + 2 (+ n_max)) * 2**-23 * ref + 1.5e-45.

NaN positions are exact, and voxels no source reaches, the last plane of every axis among them, are exactly the input.
Every test prints the largest error in units of its bound and how many voxels differ at all.  Seen on an MI355X: every
float32 result (the 37 homolog images of the option matrix, the samples and the sum of the default-size cloud, the 70-source
batch) equal to the reference in every bit; in float64 1 to 20 of 960 voxels differ per add_source case with a box of 21, by
at most 2.3e-13 on values near 1e3, 0.096 of the allowed bound; gauss_ker: up to 558 of 4 913 values differ, by 1.1e-16 at
most, 0.06 of the allowed bound.
"""
import numpy as np
import pytest

from conftest import load_golden
from harness import cloud_cases as K

pytestmark = pytest.mark.gpu

MARGIN, TINY, EPS64, EPS32 = 8.0, 2.3e-308, 2.0**-52, 2.0**-23


@pytest.fixture(scope="module")
def L():
    from imageanalysis3_amd import _lib
    _lib.check(_lib.lib().ia3_init(0))
    return _lib


@pytest.fixture(scope="module")
def V(L):
    from imageanalysis3_amd import visual_tools
    return visual_tools


@pytest.fixture(scope="module")
def S(L):
    from imageanalysis3_amd.structure_tools import chromosome
    return chromosome


@pytest.fixture(scope="module")
def gold():
    return load_golden("clouds.npz")


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def report(what, got, ref, bound):
    """Prints the largest error in units of the bound and the number of values that differ at all; True when NaN meets NaN,
    the error is within the bound everywhere and exact where the bound is 0."""
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    nan = np.isnan(ref)
    if not np.array_equal(np.isnan(got), nan):
        print(what, "NaN positions differ")
        return False
    err = np.abs(np.where(nan, 0, got).astype(np.float64) - np.where(nan, 0, ref).astype(np.float64))
    bound = np.broadcast_to(bound, err.shape)
    ratio = np.where(err > 0, err / np.where(bound > 0, bound, 1e-320), 0)
    print("%s: %d of %d values differ, largest error %.3e, %.3g of its bound" % (what, int((err > 0).sum()), err.size,
                                                                            float(err.max()) if err.size else 0.0,
                                                                            float(ratio.max()) if err.size else 0.0))
    return bool((err <= bound).all())


def bound64(shape, init, pos, h, sig, fold):
    """The float64 bound of the module's docstring, times MARGIN, per voxel; 0 where no source reaches."""
    n = K.contributing(shape, pos, sig, fold)
    S = K.np_add_sources(np.zeros(shape), pos, np.abs(h), sig, fold)
    S = np.where(np.isnan(S), 0, S)
    sig_b = np.broadcast_to(np.asarray(sig, dtype=np.float64), (len(pos), 3))
    fold_b, h_b = np.broadcast_to(fold, (len(pos),)), np.broadcast_to(np.abs(h), (len(pos),))
    hsum = np.zeros(shape)
    for i in range(len(pos)):
        hsum += h_b[i] * K.contributing(shape, pos[i:i + 1], sig_b[i:i + 1], fold_b[i:i + 1])
    return MARGIN * (3 * EPS64 * S + n * EPS64 * (np.abs(init) + S)) + TINY * hsum, n


def test_gauss_ker(V, gold):
    """s of 0, 1, 6 and 7, three sigmas and three fractional parts, a zero sigma, the defaults."""
    for name, (sig, s, disp) in K.ker_cases().items():
        got, ref = V.gauss_ker(sig, s, disp), gold[name]
        assert report(name, got, ref, MARGIN * 2 * EPS64 * np.where(np.isnan(ref), 0, ref) + TINY), name
    assert same(V.gauss_ker(), V.gauss_ker([2, 2, 2], 16, [0, 0, 0])) and V.gauss_ker().shape == (17, 17, 17)
    assert same(V.gauss_ker(np.array(K.KER_SIG), np.int64(7), np.array(K.KER_DISP)), V.gauss_ker(K.KER_SIG, 7, K.KER_DISP))
    z = V.gauss_ker(*K.ker_cases()["ker_zero_sigma"])
    assert np.isnan(z[:, :, 3]).all() and (z[:, :, [0, 1, 2, 4, 5, 6]] == 0).all()


def test_add_source(V, gold):
    """float32 and uint16 images that are not zero, both signs of h, positions inside, at -0.5, at -3.5, at shape - 0.1, at
    shape and far outside on either side of every axis, boxes of 4, 5 and 21 (larger than the image)."""
    for name, (dtype, pos, h, sig, fold) in K.source_cases().items():
        base = K.base_image(dtype)
        keep = base.copy()
        got = V.add_source(base, pos, h, sig, fold)
        assert same(base, keep), name
        f = base.astype(np.float64)
        bound, n = bound64(K.SHAPE, f, np.array([pos]), np.array([h]), sig, fold)
        assert report(name, got, gold[name], bound), name
        assert same(got[n == 0], f[n == 0]) and same(got[-1], f[-1]) and same(got[:, -1], f[:, -1]) and same(got[:, :, -1], f[:, :, -1])
    assert same(V.add_source(np.zeros((4, 5, 6)))[:3, :4, :5] > 0, np.ones((3, 4, 5), dtype=bool))      # the defaults
    pfit = np.array([150.0, 5.3, 4.6, 3.2, 100.0, 0.0, 0.0, 0.0, 0.6, 0.5, 0.4])
    u16 = K.base_image(np.uint16)
    for fn, key, sign in ((V.subtract_source, "pfit_minus", -1), (V.plus_source, "pfit_plus", 1)):
        bound, _ = bound64(K.SHAPE, u16.astype(np.float64), pfit[None, 1:4], np.array([sign * pfit[0]]), pfit[-3:], 10)
        assert report(key, fn(u16, pfit), gold[key], bound), key


def test_add_sources_equals_the_loop_and_the_reference(V, gold):
    """70 sources (two chunks of the kernel) of both signs on the float32 image: the batch is the loop of add_source bit for
    bit, device against device, in both rounding modes; the float64 result against the reference's; the last planes."""
    pos, h, sig, fold = K.multi_case()
    im = K.base_image(np.float32)
    batch64 = V.add_sources(im, pos, h, sig, fold)
    batch32 = V.add_sources(im, pos, h, sig, fold, rounding=np.float32)
    assert batch64.dtype == np.float64 and batch32.dtype == np.float32
    loop64, loop32 = im, im.copy()
    for i in range(len(pos)):
        loop64 = V.add_source(loop64, pos[i], h[i], sig[i], fold[i])
        loop32[...] = V.add_source(loop32, pos[i], h[i], sig[i], fold[i])
    assert same(batch64, loop64) and same(batch32, loop32)
    assert same(V.add_sources(im, pos, h, sig, fold), batch64) and same(V.add_sources(im, pos, h, sig, fold, rounding=np.float32), batch32)
    f = im.astype(np.float64)
    bound, n = bound64(K.SHAPE, f, pos, h, sig, fold)
    assert report("multi_f64", batch64, gold["multi_f64"], bound)
    for got, start in ((batch64, f), (batch32, im)):
        assert same(got[n == 0], start[n == 0])
        assert same(got[-1], start[-1]) and same(got[:, -1], start[:, -1]) and same(got[:, :, -1], start[:, :, -1])
    assert (n > 0).sum() > 300 and n.max() >= 8
    # all h >= 0: the float32 bound against the restatement, which equals the reference bit for bit (test_clouds_cpu.py)
    got = V.add_sources(im, pos, np.abs(h), sig, fold, rounding=np.float32)
    ref = K.np_add_sources(im, pos, np.abs(h), sig, fold, rounding=np.float32)
    assert report("multi_f32, h >= 0", got, ref, n * np.spacing(ref).astype(np.float64))
    assert same(V.add_sources(im, pos[:0], 1, [2, 2, 2]), f)          # no source at all


def test_an_image_alone_equals_the_same_image_in_a_batch(L):
    """Bit for bit: the result does not depend on the other images of the launch, and two runs agree."""
    pos, h, sig, fold = K.multi_case()
    table = L.cloud_sources(pos, h, sig, fold)
    starts = [0, 5, 5, 40, 70]
    for rounding in (None, np.float32):
        batch = L.cloud_render(table, starts, K.SHAPE, rounding=rounding)
        assert same(batch, L.cloud_render(table, starts, K.SHAPE, rounding=rounding))
        assert not batch[1].any() and batch[0].any()
        for i in range(4):
            a, b = starts[i], starts[i + 1]
            assert same(L.cloud_render(table[a:b], [0, b - a], K.SHAPE, rounding=rounding)[0], batch[i]), (rounding, i)
        with L.CloudImages(batch.nbytes) as buf:
            assert same(buf.render(table, starts, K.SHAPE, rounding=rounding), batch)
            assert same(buf.render(table[:5], [0, 5], K.SHAPE, rounding=rounding)[0], batch[0])      # zeroed again
            with pytest.raises(ValueError):
                buf.render(table, starts + [70], K.SHAPE, rounding=rounding)


def cloud_bound(cell, opt, chr_name, kept_index, ref):
    """The float32 bound of the module's docstring for one homolog of an option set."""
    allowed, per, counts, pdf, empty = opt
    kw = K.cloud_kwargs(opt)
    center = np.nanmean(np.concatenate([h for hs in cell.values() for h in hs]), axis=0)
    zxys = cell[chr_name][kept_index] - center
    valid = np.isfinite(zxys).all(1)
    pos = (kw["im_radius"] + zxys[valid]) / kw["pixel_size"]
    n = K.contributing(ref.shape, pos, [kw["gaussian_sigma"] / kw["pixel_size"]] * 3, kw["im_radius"] * 3)
    if not (counts or pdf):
        return n * np.spacing(ref).astype(np.float64), n
    return (n + 2 + (n.max() if pdf else 0)) * EPS32 * ref.astype(np.float64) + 1.5e-45 * (n > 0), n


def test_clouds_over_the_option_matrix(S, gold):
    """Homolog counts 1, 2 and 3, the homolog with exactly min_valid_spots valid loci, min_valid_per on both sides of its
    threshold, NaN loci, loci outside the grid, both normalisations, return_empty both ways, a chromosome that disappears."""
    cell = K.cell()
    for i, opt in enumerate(K.cloud_options()):
        out = S.convert_chr2Zxys_2_Cloud(cell, **K.cloud_kwargs(opt))
        assert ",".join(out) == str(gold["cloud_%d_keys" % i]), opt
        for c, arr in out.items():
            ref = gold["cloud_%d_%s" % (i, c)]
            assert arr.shape == ref.shape and arr.dtype == np.float32
            # which homologs of the cell the rows are: all with return_empty, else those the rules keep
            valid = np.isfinite(cell[c]).all(2)
            rows = [j for j in range(len(cell[c])) if opt[4] or (valid[j].sum() > K.MIN_SPOTS and valid[j].mean() >= opt[1])]
            assert len(rows) == len(ref), (opt, c)
            for k, j in enumerate(rows):
                if not ref[k].any():
                    assert not arr[k].any(), (opt, c, k)
                    continue
                bound, n = cloud_bound(cell, opt, c, j, ref[k])
                assert report("option set %d %s[%d]" % (i, c, k), arr[k], ref[k], bound), (opt, c, k)
                assert not arr[k][n == 0].any()
            assert not arr[:, -1].any() and not arr[:, :, -1].any() and not arr[..., -1].any()


def test_default_size_cloud(S, gold):
    """100**3 voxels and a box of 76 per locus, 21 loci: the sampled voxels, the last planes and the sum."""
    cell = K.default_cell()
    out = S.convert_chr2Zxys_2_Cloud(cell)
    assert list(out) == ["1"] and out["1"].shape == (1, 100, 100, 100) and out["1"].dtype == np.float32
    big = out["1"][0]
    opt = ([1, 2], 0.25, False, False, False)
    kw = dict(K.cloud_kwargs(opt), pixel_size=0.1, im_radius=5)
    center = np.nanmean(cell["1"][0], axis=0)
    n = K.contributing(big.shape, (kw["im_radius"] + (cell["1"][0] - center)) / kw["pixel_size"], [5.0] * 3, 15)
    idx = K.sample_index(big.size)
    ref = gold["big_samples"]
    assert report("default size, samples", big.ravel()[idx], ref, n.ravel()[idx] * np.spacing(ref).astype(np.float64))
    assert same(np.stack([big[-1], big[:, -1], big[:, :, -1]]), gold["big_planes"]) and not big[n == 0].any()
    # the sum of values >= 0 moves relatively no more than its terms do, n_max * 2**-23, and NumPy's pairwise float32 sum
    # of 1e6 terms rounds some 32 times on either side
    total, ref_total = np.sum(big), gold["big_sum"]
    print("sum %r, reference %r" % (total, ref_total))
    assert abs(float(total) - float(ref_total)) <= (n.max() + 32) * EPS32 * float(ref_total)


def test_list_form_equals_the_calls_per_cell(S):
    cells = K.cells_list()
    for opt in (K.cloud_options()[0], K.cloud_options()[3]):
        kw = K.cloud_kwargs(opt)
        got = S.convert_chr2Zxys_list_2_Clouds(cells, **kw)
        assert isinstance(got, list) and len(got) == len(cells)
        for cell, g in zip(cells, got):
            one = S.convert_chr2Zxys_2_Cloud(cell, **kw)
            assert list(one) == list(g) and all(same(one[c], g[c]) for c in one), opt
