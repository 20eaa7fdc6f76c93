"""Deterministic cases of the density clouds (csrc/cloud.hip), shared by scripts/make_cloud_golden.py and the tests, and a
NumPy restatement of what the reference computes (points 1 to 5) that the CPU test holds against the
fixture bit for bit.  Inputs come from the counter-based generator of ``imageanalysis3_amd.synth`` and are not stored.

The kernel gives a workgroup a 4 x 4 x 16 tile and stages 64 sources at a time; the images here are 12 x 10 x 8 (not cubic,
no multiple of the tile, several tiles on two axes) and 12**3, one case has 70 sources (two chunks), and one cloud has the
reference's default 100**3 voxels.
"""
import numpy as np

from imageanalysis3_amd import synth

# ---- gauss_ker ----------------------------------------------------------------------------------------------------------------

KER_SIG = (1.3, 2.1, 0.8)            # three different sigmas and three different fractional parts: any other pairing of
KER_DISP = (0.25, 0.6, 0.85)         # axes, sigmas and displacements gives another kernel
KER_SIZES = (0, 1, 6, 7)


def ker_cases():
    """name -> (sig, s, disp).  The zero sigma makes 0 / 0 at the centre row of one axis (NaN) and x / 0 elsewhere (0)."""
    d = {"ker_s%d" % s: (KER_SIG, s, KER_DISP) for s in KER_SIZES}
    d["ker_zero_sigma"] = ((1.5, 0.0, 2.0), 6, (0.3, 0.0, 0.7))
    d["ker_defaults"] = ((2, 2, 2), 16, (0, 0, 0))
    return d


# ---- add_source ---------------------------------------------------------------------------------------------------------------

SHAPE = (12, 10, 8)
BASE_POS = (5.3, 4.6, 3.2)
SMALL_EVEN = ((0.5, 0.4, 0.3), 6)    # s = 3: a box of 4
SMALL_ODD = ((0.7, 0.5, 0.6), 6)     # s = int(4.2) = 4: a box of 5, pos_min rounds toward zero
LARGE = ((2, 2, 2), 10)              # the defaults: a box of 21, larger than the image


def base_image(dtype):
    """A 12 x 10 x 8 image that is non-zero everywhere: uint16 counts, or float32 with a fractional part."""
    u = synth.uniform01(7, 1, np.arange(int(np.prod(SHAPE)))).reshape(SHAPE)
    if np.dtype(dtype) == np.uint16:
        return (100 + np.floor(u * 900)).astype(np.uint16)
    return (100 + np.floor(u * 900) + 0.25).astype(np.float32)


def positions():
    """The base position, and per axis: -0.5 (truncates to 0), -3.5, shape - 0.1, exactly shape, far outside on either side."""
    out = [("in", BASE_POS)]
    for k in range(3):
        for tag, v in (("m05", -0.5), ("m35", -3.5), ("edge", SHAPE[k] - 0.1), ("shape", float(SHAPE[k])), ("farlo", -1000.5),
                       ("farhi", 1000.25)):
            p = list(BASE_POS)
            p[k] = v
            out.append(("%s%d" % (tag, k), tuple(p)))
    return out


def source_cases():
    """name -> (dtype, pos, h, sig, size_fold); dtype and the sign of h alternate."""
    d, i = {}, 0
    for kname, (sig, fold) in (("even", SMALL_EVEN), ("odd", SMALL_ODD), ("large", LARGE)):
        for pname, pos in positions():
            if kname == "large" and not pname.startswith(("in", "m05", "m35", "edge1", "shape2")):
                continue
            d["src_%s_%s" % (kname, pname)] = ((np.float32, np.uint16)[i % 2], pos, (200, -37.5)[(i // 2) % 2], sig, fold)
            i += 1
    return d


def multi_case():
    """70 sources on the float32 base image: positions inside and around it, both signs of h, three kernels."""
    n = 70
    u = synth.uniform01(7, 2, np.arange(n * 5)).reshape(n, 5)
    pos = (u[:, :3] * 1.5 - 0.25) * np.array(SHAPE)
    h = np.where(u[:, 3] < 0.5, -1.0, 1.0) * (1 + np.floor(u[:, 4] * 50))
    kinds = (SMALL_EVEN, SMALL_ODD, ((1.1, 0.9, 1.4), 3))
    sig = np.array([kinds[i % 3][0] for i in range(n)], dtype=np.float64)
    fold = np.array([kinds[i % 3][1] for i in range(n)], dtype=np.float64)
    return pos, h, sig, fold


# ---- convert_chr2Zxys_2_Cloud -------------------------------------------------------------------------------------------------

PIXEL, RADIUS, MIN_SPOTS = 0.5, 3, 10


def _homolog(stream, regions, nan_every=0, spread=1.2):
    u = synth.uniform01(11, stream, np.arange(regions * 3 + 3))
    z = (u[3:].reshape(regions, 3) - 0.5) * 2 * spread + (u[:3] - 0.5)
    if nan_every:
        z[::nan_every] = np.nan
    return z


def cell():
    """chr -> (homologs, regions, 3).  c1, c2, c3: one, two and three homologs (c1 with NaN loci, c2 with loci outside the
    grid and one far outside); few: a homolog with exactly MIN_SPOTS valid loci (skipped) beside one with MIN_SPOTS + 1;
    per: 11 of 40 loci valid, 0.275, kept at min_valid_per 0.25 and skipped at 0.3, where the chromosome disappears; gone:
    two valid loci, always skipped."""
    c = {}
    c["c1"] = np.stack([_homolog(1, 30, nan_every=9)])
    c2 = np.stack([_homolog(2, 25), _homolog(3, 25)])
    c2[0, 3] = [3.4, 0.2, -0.1]          # the box is cut by the grid's end
    c2[0, 7] = [0.1, -3.3, 3.1]
    c2[1, 5] = [5.0, 0.0, 0.0]           # the box ends where the grid does: nothing is added
    c2[1, 6] = [0.0, 250.0, 0.0]
    c["c2"] = c2
    c["c3"] = np.stack([_homolog(4 + i, 16) for i in range(3)])
    few = np.stack([_homolog(8, 14), _homolog(9, 14)])
    few[0, :4] = np.nan                  # 10 valid
    few[1, :3] = np.nan                  # 11 valid
    c["few"] = few
    per = _homolog(10, 40)
    per[11:] = np.nan
    c["per"] = np.stack([per])
    gone = _homolog(12, 12)
    gone[2:] = np.nan
    c["gone"] = np.stack([gone])
    return c


def cloud_options():
    """The option sets of the fixture: (allowed_homolog_num, min_valid_per, normalize_counts, normalize_pdf, return_empty)."""
    return [([1, 2], 0.25, False, False, False), ([1, 2, 3], 0.25, True, False, False), ([1, 2], 0.3, False, True, False),
            ([1, 2, 3], 0.3, True, True, True), ([1, 2], 0.25, False, False, True), ([2], 0.25, True, True, False)]


def cloud_kwargs(opt):
    allowed, per, counts, pdf, empty = opt
    return dict(pixel_size=PIXEL, im_radius=RADIUS, gaussian_sigma=0.5, allowed_homolog_num=allowed, min_valid_spots=MIN_SPOTS,
                min_valid_per=per, normalize_counts=counts, normalize_pdf=pdf, return_empty=empty)


def cells_list():
    """Cells of the list form: the cell above, one that keeps nothing, and a small one."""
    return [cell(), {"gone": cell()["gone"]}, {"c1": cell()["c1"], "c3": cell()["c3"][:2]}]


def default_cell():
    """One homolog of 21 loci for the function's defaults: 100**3 voxels and a box of 76 per locus."""
    return {"1": np.stack([_homolog(20, 21, spread=2.0)])}


def sample_index(size, n=4096):
    """Flat indices of the sampled voxels of the default-size cloud."""
    return (synth.uniform01(99, 11, np.arange(n)) * size).astype(np.int64)


# ---- the NumPy restatement ----------------------------------------------------------------------------------------------------

def np_axis_term(n, disp, s, sig):
    """u * u over the coordinates 0 .. n - 1 of one axis."""
    with np.errstate(all="ignore"):
        u = ((np.arange(n) - np.float64(disp)) - s / 2.) / (np.float64(sig) * np.float64(sig))
        return u * u


def np_gauss_ker(sig, s, disp):
    """Point 1: kernel axis 0 pairs with entry 2, axis 1 with entry 0, axis 2 with entry 1; the sum starts with entry 0."""
    t0, t1, t2 = (np_axis_term(s + 1, disp[p], s, sig[p]) for p in (2, 0, 1))
    with np.errstate(all="ignore"):
        return np.exp(-((t1[None, :, None] + t2[None, None, :]) + t0[:, None, None]) / 2.)


def np_box(pos, s, shape):
    """Point 2, in integers: (pos_min, lo, hi) per axis."""
    pmin, lo, hi = [], [], []
    for k in range(3):
        pi = int(pos[k])
        n = s + 1
        w = pi - n // 2
        m = w if n % 2 == 0 else (w - 1 if w >= 1 else w)
        clamp = lambda p: shape[k] - 1 if p >= shape[k] else max(p, 0)
        pmin.append(m), lo.append(clamp(m)), hi.append(clamp(m + n))
    return pmin, lo, hi


def np_add_source(im, pos, h, sig, size_fold):
    """Points 2 and 3: a float64 copy of ``im`` plus the kernel times h on the clamped box."""
    out = np.array(im, dtype=np.float64)
    pos = [float(v) for v in pos]
    s = int(max(sig) * size_fold)
    ker = np_gauss_ker(sig, s, [float(-int(p)) + p for p in pos])
    pmin, lo, hi = np_box(pos, s, out.shape)
    if all(b > a for a, b in zip(lo, hi)):
        with np.errstate(all="ignore"):
            out[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] += ker[lo[0] - pmin[0]:hi[0] - pmin[0], lo[1] - pmin[1]:hi[1] - pmin[1],
                                                              lo[2] - pmin[2]:hi[2] - pmin[2]] * h
    return out


def np_add_sources(im, pos, h, sig, size_fold, rounding=None):
    """The loop of np_add_source; with ``rounding=np.float32`` the running image is rounded after every source (point 4)."""
    n = len(pos)
    h, fold = np.broadcast_to(h, (n,)), np.broadcast_to(size_fold, (n,))
    sig = np.broadcast_to(np.asarray(sig, dtype=np.float64), (n, 3))
    acc = np.array(im, dtype=np.float64 if rounding is None else rounding)
    for i in range(n):
        acc[...] = np_add_source(acc, pos[i], h[i], list(sig[i]), fold[i])
    return acc


def np_cloud(chr2Zxys, pixel_size=0.1, im_radius=5, gaussian_sigma=0.5, allowed_homolog_num=[1, 2], min_valid_spots=20,
             min_valid_per=0.25, normalize_counts=False, normalize_pdf=False, return_empty=False):
    """Point 5 around point 4."""
    center = np.nanmean(np.concatenate([h for hs in chr2Zxys.values() for h in hs]), axis=0)
    size = int(im_radius * 2 / pixel_size)
    sig = [gaussian_sigma / pixel_size] * 3
    out = {}
    for c, hs in chr2Zxys.items():
        if len(hs) not in allowed_homolog_num:
            continue
        arr = np.zeros((len(hs),) + (size,) * 3, dtype=np.float32)
        for i, zxys in enumerate(hs - center[np.newaxis, :]):
            valid = np.isfinite(zxys).all(1)
            if np.sum(valid) <= min_valid_spots or np.mean(valid) < min_valid_per:
                continue
            arr[i] = np_add_sources(arr[i], (im_radius + zxys[valid]) / pixel_size, 1, sig, im_radius * 3, rounding=np.float32)
            if normalize_counts:
                arr[i] = arr[i] / np.sum(valid)
            if normalize_pdf:
                arr[i] = arr[i] / np.sum(arr[i])
        keep = arr.any((1, 2, 3))
        if return_empty:
            out[c] = arr
        elif keep.any():
            out[c] = arr[keep]
    return out


def contributing(shape, pos, sig, size_fold):
    """Per voxel how many of the sources reach it (their clamped boxes hold it): the n of the tolerances."""
    n = np.zeros(shape, dtype=np.int64)
    sig = np.broadcast_to(np.asarray(sig, dtype=np.float64), (len(pos), 3))
    fold = np.broadcast_to(size_fold, (len(pos),))
    for i in range(len(pos)):
        _, lo, hi = np_box([float(v) for v in pos[i]], int(max(sig[i]) * fold[i]), shape)
        n[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] += 1
    return n
