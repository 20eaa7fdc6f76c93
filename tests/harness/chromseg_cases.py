"""TEST INFRASTRUCTURE — deterministic inputs of the candidate-chromosome tests: the generated stacks
(scripts/make_chromosome_golden.py stores the reference's outputs for them in tests/golden/chromosome.npz, the tests build
the stacks again) and the designed masks of the morphology and labelling tests."""
import numpy as np

# ---- generated stacks ----------------------------------------------------------------------------------------------------------
STACKS = {"small": ((12, 40, 72), 6, 11), "large": ((20, 96, 130), 14, 12)}   # shape, blobs, seed
# a second pair, of which the golden file holds nothing
FRESH = {"small": ((12, 40, 72), 6, 21), "large": ((20, 96, 130), 14, 22)}
DTYPES = ("u16", "f32")
FILT_SIZES = (3, 4)
PERCENTILES = (97.0, 90.0)
MIN_SIZES = (20, 100)


def stack(shape, n_blobs, seed, dtype="u16"):
    """Poisson(400) background with ``n_blobs`` Gaussian blobs (sigma 1.5-3.5, amplitude 1500-4000) of which 8 % of the
    voxels above half the amplitude are knocked out to the background level; every other blob is cut off at 45 % of its
    amplitude, so its core is flat: the range filter is small there and the thresholded seed is a closed shell around a
    cavity, which the hole filling has to fill.  "u16": uint16; "f32": the same counts divided by 3 in float32, so that
    neither the voxels nor the plane medians are whole numbers."""
    rng = np.random.RandomState(seed)
    Z, X, Y = shape
    im = rng.poisson(400., size=shape).astype(np.float64)
    z, x, y = np.meshgrid(np.arange(Z), np.arange(X), np.arange(Y), indexing="ij")
    for k in range(n_blobs):
        c = np.array([rng.uniform(3, Z - 3), rng.uniform(6, X - 6), rng.uniform(6, Y - 6)])
        s = rng.uniform(1.5, 3.5, size=3) * np.array([0.6, 1.0, 1.0])
        a = rng.uniform(1500, 4000)
        g = a * np.exp(-0.5 * (((z - c[0]) / s[0]) ** 2 + ((x - c[1]) / s[1]) ** 2 + ((y - c[2]) / s[2]) ** 2))
        hit = (g > 0.5 * a) & (rng.rand(*shape) < 0.08)
        g[hit] = 0
        if k % 2:
            g = np.minimum(g, 0.45 * a)
        im += g
    im = np.clip(np.round(im), 0, 65535).astype(np.uint16)
    if dtype == "u16":
        return im
    return (im.astype(np.float32) / np.float32(3)).astype(np.float32)


def generated(name, dtype, fresh=False):
    shape, n, seed = (FRESH if fresh else STACKS)[name]
    return stack(shape, n, seed, dtype)


def golden_cases():
    """(key, stack name, dtype, filt_size, percentile, min_label_size) of every entry of tests/golden/chromosome.npz"""
    out = []
    for name in STACKS:
        for dt in DTYPES:
            for fs in FILT_SIZES:
                for per in PERCENTILES:
                    for ms in MIN_SIZES:
                        out.append(("%s_%s_f%d_p%g_m%d" % (name, dt, fs, per, ms), name, dt, fs, per, ms))
    out.append(("small_u16_f3_p99.5_m20", "small", "u16", 3, 99.5, 20))
    return out


def pack_labels(kept):
    """A uint16 label volume as (bits of label > 0 packed along y, the labels of the set voxels in raster order)."""
    return np.packbits(kept > 0, axis=-1), kept[kept > 0].astype(np.uint16)


def unpack_labels(bits, values, shape):
    m = np.unpackbits(bits, axis=-1, count=shape[-1]).astype(bool)
    out = np.zeros(shape, np.uint16)
    out[m] = values
    return out


# ---- designed masks ------------------------------------------------------------------------------------------------------------
MASK_SHAPES = ((9, 37, 131), (20, 70, 200))


def _shell(m, lo, hi):
    """the one-voxel-thick wall of the box lo <= (z, x, y) < hi"""
    m[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = True
    m[lo[0] + 1:hi[0] - 1, lo[1] + 1:hi[1] - 1, lo[2] + 1:hi[2] - 1] = False


def masks(shape):
    """name -> bool mask of ``shape`` (every axis longer than one labelling tile, rows of three words that are no
    multiple of 64)."""
    Z, X, Y = shape
    d = {}
    d["empty"] = np.zeros(shape, bool)
    d["full"] = np.ones(shape, bool)
    m = np.zeros(shape, bool)
    m[Z // 2, X // 2, Y // 2] = True
    d["one"] = m
    m = np.zeros(shape, bool)   # the corners and the middle of every face
    for z in (0, Z - 1):
        for x in (0, X - 1):
            for y in (0, Y - 1):
                m[z, x, y] = True
    m[0, X // 2, Y // 2] = m[Z - 1, X // 2, Y // 2] = True
    m[Z // 2, 0, Y // 2] = m[Z // 2, X - 1, Y // 2] = True
    m[Z // 2, X // 2, 0] = m[Z // 2, X // 2, Y - 1] = True
    d["faces"] = m
    m = np.zeros(shape, bool)   # blocks that touch by an edge (first pair) and by a corner (second pair) only
    m[2:4, 2:8, 2:6] = True
    m[4:6, 8:12, 2:6] = True
    m[2:4, 20:24, 60:64] = True
    m[4:6, 24:28, 64:70] = True
    d["edge_corner"] = m
    m = np.zeros(shape, bool)   # one path: every other row of every other plane, joined at alternating ends
    xl = (X - 1) // 2 * 2
    for z in range(0, Z, 2):
        m[z, 0:xl + 1:2, :] = True
        for k, x in enumerate(range(1, xl, 2)):
            m[z, x, Y - 1 if k % 2 == 0 else 0] = True
        if z + 1 < Z and z + 2 < Z:
            m[z + 1, 0 if (z // 2) % 2 else xl, 0 if (z // 2) % 2 else Y - 1] = True
    d["serpentine"] = m
    m = np.zeros(shape, bool)   # teeth along z that join in the last plane only
    m[:, ::2, ::2] = True
    m[Z - 1] = True
    d["comb"] = m
    m = np.zeros(shape, bool)
    _shell(m, (2, 5, 5), (8, 15, 75))
    d["shell"] = m
    m = m.copy()
    m[2, 10, 40] = False
    d["shell_leak"] = m
    m = np.zeros(shape, bool)   # the cavity is open towards the face z = 0
    m[0:6, 20:30, 40:110] = True
    m[0:5, 21:29, 41:109] = False
    d["shell_face"] = m
    m = np.zeros(shape, bool)
    _shell(m, (1, 3, 60), (8, 33, 128))
    inner = np.zeros(shape, bool)
    _shell(inner, (3, 8, 66), (6, 28, 120))
    d["nested"] = m | inner
    z, x, y = np.meshgrid(np.arange(Z), np.arange(X), np.arange(Y), indexing="ij")
    d["checker"] = (z + x + y) % 2 == 0
    rng = np.random.RandomState(Z * 1000 + X)
    d["random"] = rng.rand(*shape) < 0.62   # hundreds of irregular components
    d["dense"] = rng.rand(*shape) < 0.93    # dense enough for an erosion by ball(2) to leave something
    d["blobs"] = _blob_mask(shape)
    return d


def _blob_mask(shape):
    """a thresholded generated stack, cropped or tiled to ``shape``: irregular objects of many sizes"""
    im = generated("large", "u16")
    reps = [int(np.ceil(s / float(t))) for s, t in zip(shape, im.shape)]
    return np.tile(im, reps)[:shape[0], :shape[1], :shape[2]] > 470


def checkerboard(shape):
    z, x, y = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    return (z + x + y) % 2 == 0


OVERFLOW_SHAPE = (8, 96, 200)   # 76 800 components as a checkerboard: more than uint16 labels hold
