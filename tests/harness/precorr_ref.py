"""Inputs and rule statements for the edge tests of the elementwise pre-corrections (csrc/corrections.hip,
csrc/hotpix.hip).  NumPy only.

The fixture tests/golden/precorr_edges.json (scripts/make_precorr_edge_golden.py) holds one CRC32 per case and output,
as the reference's own functions returned them, plus the candidate counts of the hot-pixel cases; the inputs are
regenerated here.  ``CASES`` names every case once: the golden script, tests/test_precorrection_edges_cpu.py and
tests/test_gpu_precorrection_edges.py all walk it, and ``oracle(key)`` is np_oracle's result for it.

Rules stated here (np_oracle stays the reference of every comparison; these only say what the kernels document):

  to_u16             float -> uint16 as every one of these kernels ends: truncate toward zero and keep the low 16 bits
                     of the int32 where |t| < 2^31, else (inf and NaN included) 0
  bleed_sequential   products in the profile dtype, summed left to right in channel order, clipped, then cast

There is deliberately no NaN-less min/max rescale here: the reference of the rescale variants is
np_oracle.daxp_illumination / daxp_bleedthrough, whose np.min / np.max propagate NaN.
"""
import functools
import zlib
from collections import OrderedDict

import numpy as np

import np_oracle as O

HOT_CAP = 16384   # entries of the device candidate list (csrc/hotpix.hip); one more takes the host fallback
# float -> uint16 edge values: in range, negative, just below / at / above 2^16, the last float32 below 2^31, beyond
# int32, beyond int64, infinities, NaN, negative zero
CAST_EDGES = [70000, -1.5, 65535.9, 65536, 131071.7, -65536.2, 2147483520, 3e9, -3e9, 1e10, 1e19,
              np.inf, -np.inf, np.nan, -0.0]


def crc(a):
    return int(zlib.crc32(np.ascontiguousarray(a).tobytes()))


def to_u16(t):
    t = np.asarray(t).astype(np.float64)
    ok = np.abs(t) < 2147483648.0                      # False for NaN
    i = np.trunc(np.where(ok, t, 0.0)).astype(np.int64)
    return (i & 0xFFFF).astype(np.uint16)


def saturating_u16(t):
    """What a saturating conversion would give instead (NaN -> 0): only to show that the inputs tell the two apart."""
    t = np.asarray(t).astype(np.float64)
    return np.clip(np.trunc(np.where(np.isnan(t), 0.0, t)), 0, 65535).astype(np.uint16)


# ---- hot pixels ------------------------------------------------------------------------------------------------

def hot_field(shape, seed, p_hot):
    """uint16 stack, constant over z up to noise in [0, 4): each column is hot-valued (log-uniform in [2000, 60000])
    with probability ``p_hot``, else background in [5, 50).  Dense enough that hot columns touch (later candidates see
    earlier replacements) and that the uint16 neighbour sums wrap."""
    rng = np.random.RandomState(seed)
    Z, X, Y = shape
    hot = rng.rand(X, Y) < p_hot
    val = np.exp(rng.uniform(np.log(2000.), np.log(60000.), size=(X, Y)))
    bg = rng.uniform(5., 50., size=(X, Y))
    base = np.where(hot, val, bg).astype(np.uint16)
    return (base[None] + rng.randint(0, 4, size=shape)).astype(np.uint16)


def lattice_field(n_extra):
    """(2, 258, 258), background 10, 1000 at every (2i+1, 2j+1), 0 <= i, j < 128: exactly HOT_CAP isolated interior hot
    columns; ``n_extra = 1`` adds one at (2, 2)."""
    im = np.full((2, 258, 258), 10, np.uint16)
    im[:, 1:256:2, 1:256:2] = 1000
    if n_extra:
        im[:, 2, 2] = 1000
    return im


def single_hot():
    """(4, 3, 3): the only interior column is hot."""
    im = (20 + np.arange(36, dtype=np.uint16).reshape(4, 3, 3) % 7).astype(np.uint16)
    im[:, 1, 1] = [3000, 3001, 2999, 3003]
    return im


def border_hot():
    """(4, 9, 11): one hot column on each border (rows and columns apart, so that none shades another through the
    wrap-around of np.roll) and none inside."""
    rng = np.random.RandomState(3)
    im = rng.randint(20, 30, size=(4, 9, 11)).astype(np.uint16)
    for (x, y) in ((0, 3), (8, 5), (2, 0), (6, 10)):
        im[:, x, y] = 5000
    return im


def hot_candidates(im, hot_pix_th=0.5, hot_th=4):
    """The reference's candidate columns of ``im`` (np.where order), in the arithmetic of ``im.dtype``: (xs, ys)."""
    conv = (np.roll(im, 1, 1) + np.roll(im, -1, 1) + np.roll(im, 1, 2) + np.roll(im, 1, 2)) / 4
    return np.where(np.sum(im > hot_th * conv, 0) > hot_pix_th * im.shape[0])


def wrapping_sums(im):
    """Per plane of a uint16 stack: how many of the reference's four-neighbour sums exceed 65535, so wrap in uint16."""
    w = im.astype(np.int64)
    full = np.roll(w, 1, 1) + np.roll(w, -1, 1) + 2 * np.roll(w, 1, 2)
    return [int(n) for n in (full > 65535).sum(axis=(1, 2))]


def interior(xs, ys, shape):
    return (xs > 0) & (ys > 0) & (xs < shape[1] - 1) & (ys < shape[2] - 1)


def hot_replace(im, xs, ys):
    """The reference's replacement loop over the given candidates, in the given order."""
    nim = im.copy()
    for x, y in zip(xs, ys):
        if 0 < x < im.shape[1] - 1 and 0 < y < im.shape[2] - 1:
            nim[:, x, y] = (nim[:, x + 1, y] + nim[:, x - 1, y] + nim[:, x, y + 1] + nim[:, x, y - 1]) / 4
    return nim


HOT_FIELDS = OrderedDict([
    ("rand_mid", (lambda: hot_field((5, 200, 203), 11, 0.3), 0.5, 4)),      # device list, thousands of candidates
    ("rand_big", (lambda: hot_field((3, 341, 343), 7, 0.3), 0.5, 4)),       # more than HOT_CAP: host fallback
    ("lattice0", (lambda: lattice_field(0), 0.5, 4)),                        # exactly HOT_CAP: device list
    ("lattice1", (lambda: lattice_field(1), 0.5, 4)),                        # HOT_CAP + 1: host fallback
    ("single", (single_hot, 0.5, 4)),
    ("border", (border_hot, 0.5, 4)),
    ("th_low", (lambda: hot_field((5, 200, 203), 11, 0.3), 0.3, 2.5)),      # non-integer hot_th
    ("th_high", (lambda: hot_field((5, 200, 203), 11, 0.3), 0.75, 6)),
    # a hot_th that float32 cannot hold: the float32 arithmetic multiplies by float32(2.3), the uint16 one by the double
    ("th_frac", (lambda: hot_field((5, 200, 203), 11, 0.3), 0.4, 2.3)),
])
RANDOM_HOT = ("rand_mid", "rand_big")


# ---- illumination ----------------------------------------------------------------------------------------------

# planted profile entries, at the first plane positions in row-major order (as many as the plane holds)
PLANTED = [0.0,       # under a zero voxel: 0/0 = NaN
           0.0,       # under non-zero voxels: inf
           -0.0,      # -inf under 65535, NaN under 0
           1e-3,      # quotients in [65536, 2^31): wrap
           3.05e-5,   # 65535 / 3.05e-5 is just above 2^31, 65000 / 3.05e-5 just below
           2e-5,      # >= 2^31 for voxels above 42949
           1e-30,     # >= 2^31 for every non-zero voxel
           -0.7,      # negative quotients: wrap from below
           np.nan, np.inf]
ILLUM_SHAPES = ((4, 17, 19), (3, 1, 5), (4, 16, 20), (2, 2, 2))   # scalar kernel (odd planes), four-wide kernel, tiny
DTYPES = OrderedDict([("f32", np.float32), ("f64", np.float64)])


def edge_profile(X, Y, dtype, seed):
    rng = np.random.RandomState(seed)
    pf = (0.6 + 0.4 * rng.rand(X, Y)).astype(dtype)
    n = min(len(PLANTED), X * Y)
    pf.reshape(-1)[:n] = np.array(PLANTED[:n], dtype=dtype)
    return pf


def edge_image(shape, seed):
    """Full-range uint16 stack with the voxels the planted profile entries need: a zero column under the first, non-zero
    ones under the second, 65535 in plane 0 (and 65000, 0 in the next planes) under the others."""
    rng = np.random.RandomState(seed + 1000)
    im = rng.randint(0, 65536, size=shape).astype(np.uint16)
    flat = im.reshape(shape[0], -1)
    n = min(len(PLANTED), flat.shape[1])
    flat[:, 0] = 0
    if n > 1:
        flat[:, 1] = np.maximum(flat[:, 1], 1)
    for k in range(2, n):
        flat[0, k] = 65535
        if shape[0] > 1:
            flat[1, k] = 65000
        if shape[0] > 2:
            flat[2, k] = 0
    return im


def quotient_census(q):
    """How many quotients sit in each class of the cast rule."""
    q = np.asarray(q, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return dict(wrap=int(((q >= 65536) & (q < 2147483648.0)).sum()), overflow=int((q >= 2147483648.0).sum()),
                    negative=int((q < 0).sum()), nan=int(np.isnan(q).sum()))


# ---- bleedthrough ----------------------------------------------------------------------------------------------

BLEED_CASES = [(C, (3, 17, 19)) for C in (1, 2, 3, 4, 8)] + [(3, (3, 16, 20)), (4, (3, 16, 20))]


def mix_profile(C, X, Y, dtype, seed):
    """eye(C) + 0.3 randn per pixel, with one NaN, one +inf and one -inf entry (at different pixels)."""
    rng = np.random.RandomState(seed)
    pf = (np.eye(C)[:, :, None, None] + 0.3 * rng.randn(C, C, X, Y)).astype(dtype)
    pf[0, C - 1].reshape(-1)[1] = np.nan
    pf[C - 1, 0].reshape(-1)[3] = np.inf
    pf[C // 2, C // 2].reshape(-1)[5] = -np.inf
    return pf


def mix_images(C, shape, seed):
    rng = np.random.RandomState(seed + 2000)
    ims = [rng.randint(0, 65536, size=shape).astype(np.uint16) for _ in range(C)]
    ims[0][0, 0, :4] = [0, 65535, 0, 0]      # 0 * NaN, 0 * inf among the products
    return ims


def bleed_sequential(ims, prof, order=None):
    """The kernels' stated arithmetic.  ``order``: the channel order of the sum (default 0 .. C-1)."""
    P = prof.dtype.type
    order = list(range(len(ims))) if order is None else list(order)
    outs = []
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(len(ims)):
            s = ims[order[0]].astype(P) * prof[a, order[0]]
            for j in order[1:]:
                s = s + ims[j].astype(P) * prof[a, j]
            s = np.where(s > P(65535), P(65535), s)
            s = np.where(s < P(0), P(0), s)
            outs.append(to_u16(s))
    return outs


# ---- rescale variants (DaxProcesser steps) ---------------------------------------------------------------------

RESCALE_SHAPES = ((3, 17, 19), (3, 16, 20))
SMALL_SHAPE = (1, 3, 5)          # fewer voxels than one block: most min / max partials stay at +-inf
RESCALE_KINDS = ("ordinary", "constant", "inf", "nan", "nan_far")
# The min / max kernels reduce voxel v in block (v / 256) % 1024, inside each block by a tree over shared memory, and then
# the 1024 block partials by a second tree (minmax_final_k).  Slot 0 of a tree is only ever the running value, and the
# plain `a < b ? a : b` keeps a NaN there too: a NaN in the first block's partial cannot tell whether the second tree
# propagates it.  "nan" plants its column at pixel NAN_NEAR (block 0 holds a NaN voxel), "nan_far" at pixel NAN_FAR,
# where every NaN voxel lies in a later block and the first block's partial stays finite.
MINMAX_BLOCK = 256
NAN_NEAR, NAN_FAR = 3, 300


def nan_voxels(kind, shape):
    """Flat voxel indices of the NaN column that ``kind`` plants in a stack of ``shape``."""
    pix = {"nan": NAN_NEAR, "nan_far": NAN_FAR}[kind]
    assert pix < shape[1] * shape[2]
    return [z * shape[1] * shape[2] + pix for z in range(shape[0])]


def rescale_illum_input(kind, shape, dtype, seed=5):
    rng = np.random.RandomState(seed)
    Z, X, Y = shape
    im = rng.randint(0, 65536, size=shape).astype(np.uint16)
    pf = (0.6 + 0.4 * rng.rand(X, Y)).astype(dtype)
    if kind == "constant":                      # max == min: 0/0 everywhere under rescale
        im[:] = 1234
        pf[:] = 0.8
    elif kind == "inf":                         # x/0
        pf.reshape(-1)[3] = 0
        im.reshape(Z, -1)[:, 3] = 4321
    elif kind in ("nan", "nan_far"):            # a single 0/0 column, nothing infinite
        pix = NAN_NEAR if kind == "nan" else NAN_FAR
        pf.reshape(-1)[pix] = 0
        im.reshape(Z, -1)[:, pix] = 0
    return im, pf


def rescale_bleed_input(kind, C, shape, dtype, seed=6):
    rng = np.random.RandomState(seed + C)
    Z, X, Y = shape
    ims = [rng.randint(0, 65536, size=shape).astype(np.uint16) for _ in range(C)]
    pf = (np.eye(C)[:, :, None, None] + 0.3 * rng.randn(C, C, X, Y)).astype(dtype)
    if kind == "constant":
        for j in range(C):
            ims[j][:] = 1000 * (j + 1)
        pf[:] = (np.eye(C) + 0.25)[:, :, None, None]
    elif kind == "inf":                         # output 0 holds +inf, the others stay ordinary
        pf[0, 0].reshape(-1)[3] = np.inf
        ims[0].reshape(Z, -1)[:, 3] = 4321
    elif kind in ("nan", "nan_far"):            # the last output holds one NaN column
        pf[C - 1, 0].reshape(-1)[NAN_NEAR if kind == "nan" else NAN_FAR] = np.nan
    return ims, pf


# ---- z shift ---------------------------------------------------------------------------------------------------

def _zero_plane():
    rng = np.random.RandomState(8)
    im = rng.randint(100, 4000, size=(6, 4, 6)).astype(np.uint16)
    im[2] = 0
    im[2, 0, :3] = [7, 900, 65535]              # median still 0: x/0 next to 0/0
    return im


ZSHIFT = OrderedDict([
    # 2 (Z + 1) = 132 selection problems and Z + 1 = 66 medians: second 64-thread blocks; odd plane, odd stack
    ("z65", lambda: np.random.RandomState(1).randint(100, 4000, size=(65, 5, 7)).astype(np.uint16)),
    ("z130", lambda: np.random.RandomState(2).randint(0, 65536, size=(130, 3, 3)).astype(np.uint16)),   # even stack
    ("f32neg", lambda: (np.random.RandomState(3).randn(5, 6, 7) * 50).astype(np.float32)),   # negative keys, wraps
    ("zero_plane", _zero_plane),                                                              # even plane
    ("const_planes", lambda: (100 + 10 * np.arange(6, dtype=np.uint16))[:, None, None] * np.ones((1, 4, 6), np.uint16)),
    ("tiny", lambda: np.array([[[5, 9]], [[300, 2]], [[65535, 65535]]], np.uint16)),
])


# ---- the cases -------------------------------------------------------------------------------------------------

def _shape_tag(shape):
    return "x".join(str(int(v)) for v in shape)


def _build_cases():
    c = OrderedDict()
    for shape in ILLUM_SHAPES:
        for dt in DTYPES:
            c["illum/%s/%s" % (_shape_tag(shape), dt)] = ("illum", shape, dt)
    for C, shape in BLEED_CASES:
        for dt in DTYPES:
            c["bleed/C%d/%s/%s" % (C, _shape_tag(shape), dt)] = ("bleed", C, shape, dt)
    for r in (1, 0):
        for dt in DTYPES:
            for shape, kinds in [(s, RESCALE_KINDS) for s in RESCALE_SHAPES] + [(SMALL_SHAPE, ("ordinary", "nan"))]:
                for kind in kinds:
                    c["illum_rescale/%s/%s/%s/r%d" % (kind, _shape_tag(shape), dt, r)] = ("illum_rescale", kind, shape, dt, r)
                    for C in (2, 3):
                        c["bleed_rescale/%s/C%d/%s/%s/r%d" % (kind, C, _shape_tag(shape), dt, r)] = \
                            ("bleed_rescale", kind, C, shape, dt, r)
    for name in HOT_FIELDS:
        for arith in ("u16", "f32"):
            c["hot/%s/%s" % (name, arith)] = ("hot", name, arith)
    for name in ZSHIFT:
        c["zshift/%s" % name] = ("zshift", name)
    return c


CASES = _build_cases()


def keys(kind):
    return [k for k, v in CASES.items() if v[0] == kind]


def inputs(key):
    """The arguments of a case: illum -> (im, profile); bleed -> (ims, profile); *_rescale -> (im | ims, profile,
    rescale); hot -> (im in the arithmetic's dtype, hot_pix_th, hot_th); zshift -> (im,)."""
    spec = CASES[key]
    kind = spec[0]
    if kind == "illum":
        _, shape, dt = spec
        return edge_image(shape, 1), edge_profile(shape[1], shape[2], DTYPES[dt], 1)
    if kind == "bleed":
        _, C, shape, dt = spec
        return mix_images(C, shape, 2), mix_profile(C, shape[1], shape[2], DTYPES[dt], 2)
    if kind == "illum_rescale":
        _, k, shape, dt, r = spec
        return rescale_illum_input(k, shape, DTYPES[dt]) + (bool(r),)
    if kind == "bleed_rescale":
        _, k, C, shape, dt, r = spec
        return rescale_bleed_input(k, C, shape, DTYPES[dt]) + (bool(r),)
    if kind == "hot":
        _, name, arith = spec
        make, hot_pix_th, hot_th = HOT_FIELDS[name]
        im = make()
        return (im if arith == "u16" else im.astype(np.float32)), hot_pix_th, hot_th
    if kind == "zshift":
        return (ZSHIFT[spec[1]](),)
    raise KeyError(key)


@functools.lru_cache(maxsize=None)
def oracle(key):
    """np_oracle's outputs for a case, as a tuple of read-only uint16 arrays (computed once per process).  A hot-pixel
    case in float32 arithmetic is the chain's call ``Remove_Hot_Pixels(im.astype(np.float32), dtype=np.uint16)``."""
    kind = CASES[key][0]
    a = inputs(key)
    with np.errstate(all="ignore"):
        if kind == "illum":
            outs = [O.illumination_correction(*a)]
        elif kind == "bleed":
            outs = O.bleedthrough_correction(*a)
        elif kind == "illum_rescale":
            outs = [O.daxp_illumination(a[0], a[1], a[2])]
        elif kind == "bleed_rescale":
            outs = O.daxp_bleedthrough(a[0], a[1], a[0][0].shape, a[2])
        elif kind == "hot":
            outs = [O.remove_hot_pixels(a[0], dtype=np.uint16, hot_pix_th=a[1], hot_th=a[2]).astype(np.uint16)]
        else:
            outs = [O.z_shift_correction(a[0])]
    for o in outs:
        assert o.dtype == np.uint16
        o.setflags(write=False)
    return tuple(outs)


def n_diff(got, ref):
    """Differing voxels of two arrays of one shape (what a failed bit-exact comparison reports)."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (got.shape, got.dtype, ref.shape, ref.dtype)
    return int((got != ref).sum())
