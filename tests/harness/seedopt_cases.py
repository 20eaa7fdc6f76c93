"""Inputs of the seeding-option tests (tests/test_seed_options_cpu.py, tests/test_gpu_seed_options.py,
scripts/make_seedopt_golden.py): seeded from ``imageanalysis3_amd.synth``'s hash generator, nothing stored but a CRC.

The golden cases of meta.json cannot tell the options of ``get_seeds`` apart: their spots are isolated blobs, so every
window size, hot-column threshold and edge distance returns the same list.  The field made here separates them.

* Background ``400 + 5 z + 2 x + 3 y + 20 noise``.  The slope keeps the background filter's output from settling into
  plateaus on uint16, where ``min_ft != min_im`` would reject almost every spot.
* Spike pairs, one per cell of an 11-voxel grid in the middle plane: a spike of ~20000 and a dimmer one of ~14000 at
  offset ``s * d`` (d = 1..4, s = +1 / -1) along z, x, y and the diagonal.  The dimmer spike is a local maximum of window
  W exactly when the brighter one lies outside ``[-(W // 2), W - W // 2 - 1]`` of it, so every W in 1..8 keeps another
  set, and the ``+d`` / ``-d`` twins tell an even window's two sides apart.
* Hot columns with 1..5 spikes at planes far apart: ``hot_pixel_th`` = 1..6 each remove another number of them.
* Edge spikes at coordinate ``e`` and at ``size - e`` (e = 0..6) of every axis: the reference keeps ``c >= d`` and
  ``c <= size - d``, which is not symmetric.
* Every spike has its own height, so a truncation by ``max_num_seeds`` never cuts through a tie.
"""
import zlib

import numpy as np

from imageanalysis3_amd import synth

MAIN_SHAPE = (25, 76, 96)      # Z = 25: a depth built into the library; Y a multiple of 32: the fused detector runs
RAGGED_SHAPE = (11, 70, 83)    # Z < 16; no multiple of any tile
NOISE_SHAPE = (25, 160, 192)   # the sloped noise alone: more candidates than the device finish takes
FIN_CAP = 32768                # seed.hip: candidates the device finish looks at
FIN_KEYS = 16384               # ... of which at most this many may pass the chosen level
DTYPES = ("float32", "uint16")

# (axis or "diag", distance, sign) of the dimmer spike of each pair
PAIR_SPECS = [(ax, d, s) for ax in range(3) for d in (1, 2, 3, 4) for s in (+1, -1)] + \
             [("diag", d, s) for d in (1, 2, 3, 4) for s in (+1, -1)]
HOT_PLANES = (2, 7, 12, 17, 22)

BASE = dict(use_dynamic_th=False, remove_hot_pixel=False, min_edge_distance=0, th_seed=500)
FILT_SIZES = tuple(range(1, 9))
FRONT_WIDTHS = (0, 0.75, 1.0)
HOT_THS = tuple(range(0, 7))
EDGE_DISTANCES = (0, 1, 2, 2.5, 3, 4, 5, 6, 7, 13)
BACK_WIDTHS = (0, 0.7, 0.9, 8.0, 8.2, 15.7, 16)   # radii 0 (off), 3, 4, 32, 33, 63, 64: the switch points of the lazy path
# background off or narrower than the front filter: the heights are <= 0.  The largest of -1, -10, -100, ... that keeps
# at least 50 seeds for both widths and both dtypes (-1 keeps 23)
BACK_OFF_TH = -10
# a threshold above every height (the tallest is ~4100 behind the default filters): of the levels 4000 * (1 - i / 7) the
# first with 60 seeds is i = 4, the middle one
DYNAMIC = dict(th_seed=4000, use_dynamic_th=True, dynamic_niters=7, min_dynamic_seeds=60, remove_hot_pixel=False,
               min_edge_distance=0)
DYNAMIC_LEVEL = 4

_made = {}


def crc(a):
    return int(zlib.crc32(np.ascontiguousarray(a).tobytes()))


def pair_cells(shape):
    Z, X, Y = shape
    return [(Z // 2, x, y) for x in range(12, X - 8, 11) for y in range(10, Y - 6, 11)]


def pairs(shape):
    """[(spec, bright (z, x, y), dim (z, x, y))] of the field of ``shape``."""
    cells = pair_cells(shape)
    assert len(cells) >= len(PAIR_SPECS), (len(cells), len(PAIR_SPECS))
    out = []
    for c, (ax, d, s) in zip(cells, PAIR_SPECS):
        off = np.array([1, 1, 1]) * d * s if ax == "diag" else np.eye(3, dtype=int)[ax] * d * s
        out.append(((ax, d, s), tuple(int(v) for v in c), tuple(int(v) for v in np.array(c) + off)))
    return out


def _background64(shape, seed, noise):
    z, x, y = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    return 400 + 5.0 * z + 2.0 * x + 3.0 * y + synth.background(shape, seed, bg=0.0, noise=noise)


def _field64(shape, seed, hot, edges):
    Z, X, Y = shape
    im = _background64(shape, seed, 20.0)
    k = 0   # every spike 37 above the one before: no two heights are equal

    def add(pos, h):
        nonlocal k
        im[pos] += h + 37 * k
        k += 1

    for _, bright, dim in pairs(shape):
        add(bright, 20000)
        add(dim, 14000)
    zc = Z // 2
    if hot:
        for n in range(1, 6):
            for zz in HOT_PLANES[:n]:
                add((zz, 4, 6 + 14 * n), 9000)
    if edges:   # spikes e voxels from the low faces and at size - e from the high faces
        for e in range(0, 7):
            add((e, X - 5, 8 + 12 * e), 6000)
            add((zc + 6, e, 8 + 12 * e), 6000)
            add((zc - 6, 20 + 8 * e, e), 6000)
            if e:
                add((Z - e, X - 5, 14 + 12 * e), 6000)
                add((zc + 6, X - e, 14 + 12 * e), 6000)
                add((zc - 6, 24 + 8 * e, Y - e), 6000)
    return im


def _cast(im64, dtype):
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        return im64.astype(np.float32)
    assert im64.min() >= 0 and im64.max() < 65535
    return im64.astype(np.uint16)   # truncation, as a camera's counts


def stack(name, dtype):
    """``main`` (pairs, hot columns, edge spikes), ``ragged`` (pairs only) or ``noise`` (the background alone); made once, read-only."""
    key = (name, np.dtype(dtype).name)
    if key not in _made:
        if name == "main":
            im = _cast(_field64(MAIN_SHAPE, 7, True, True), dtype)
        elif name == "ragged":
            im = _cast(_field64(RAGGED_SHAPE, 8, False, False), dtype)
        elif name == "noise":
            im = _cast(_background64(NOISE_SHAPE, 9, 30.0), dtype)
        else:
            raise KeyError(name)
        im.setflags(write=False)
        _made[key] = im
    return _made[key]


def golden_cases():
    """{key: (stack name, get_seeds options)} of the tables of tests/golden/seedopt.npz, per dtype ``<dtype>_<key>``."""
    c = {}
    for g in (0, 0.75):
        for W in FILT_SIZES:
            c["w%d_g%s" % (W, g)] = ("main", dict(BASE, filt_size=W, gfilt_size=g))
    for t in HOT_THS:
        c["hot%d" % t] = ("main", dict(BASE, remove_hot_pixel=True, hot_pixel_th=t))
    for d in EDGE_DISTANCES:
        c["edge%s" % d] = ("main", dict(BASE, min_edge_distance=d))
    for b in BACK_WIDTHS:
        c["back%s" % b] = ("main", dict(BASE, background_gfilt_size=b, th_seed=BACK_OFF_TH if b < 0.75 else 500))
    c["dynamic"] = ("main", dict(DYNAMIC))
    return c


def table_i16(t):
    """(N, 4) float64 seed table -> (int16 coordinates (N, 3), float32 heights (N,)), both exact here."""
    t = np.asarray(t, dtype=np.float64).reshape(-1, 4)
    zxy, h = t[:, :3].astype(np.int16), t[:, 3].astype(np.float32)
    assert np.array_equal(zxy, t[:, :3]) and np.array_equal(h.astype(np.float64), t[:, 3])
    return zxy, h


def golden_table(g, dtype, key):
    """The (N, 4) float64 table of a case of tests/golden/seedopt.npz."""
    k = "%s_%s" % (np.dtype(dtype).name, key)
    return np.concatenate([g[k + "_zxy"].astype(np.float64), g[k + "_h"].astype(np.float64)[:, None]], axis=1).reshape(-1, 4)


def as_set(t):
    """A seed table as a frozenset of (z, x, y, h) rows."""
    return frozenset(map(tuple, np.asarray(t, dtype=np.float64).reshape(-1, 4).tolist()))


def check_discrimination(dtype, run):
    """The conditions that make the field tell the options apart, on ``run(stack name, **options) -> (N, 4) table``
    (the reference in scripts/make_seedopt_golden.py, the oracle in tests/test_seed_options_cpu.py).  A kernel that
    ignored the window size, the hot-column threshold, the edge distance or the background width cannot meet a test
    built on tables that differ in all of them."""
    for name in ("main", "ragged"):
        for g in FRONT_WIDTHS:
            sets = [as_set(run(name, **dict(BASE, filt_size=W, gfilt_size=g))) for W in FILT_SIZES]
            assert len(sets[0]) == 0, (name, g)                       # W = 1: every voxel is its window's minimum
            assert len(set(sets)) == len(FILT_SIZES), (name, dtype, g, [len(s) for s in sets])
        # an even window reaches W / 2 voxels down and W / 2 - 1 up: of the twins at distance W / 2 the one below its
        # brighter spike sees it, the one above does not
        for W in (2, 4, 6, 8):
            zxy = {tuple(int(v) for v in r[:3]) for r in run(name, **dict(BASE, filt_size=W, gfilt_size=0))}
            dims = {(ax, s): dim for (ax, d, s), _, dim in pairs(stack(name, dtype).shape) if d == W // 2}
            for ax in (0, 1, 2, "diag"):
                assert dims[(ax, -1)] in zxy and dims[(ax, +1)] not in zxy, (name, dtype, W, ax)
    n_hot = [len(run("main", **dict(BASE, remove_hot_pixel=True, hot_pixel_th=t))) for t in HOT_THS]
    assert n_hot[0] == 0 and n_hot[1] == 0 and len(set(n_hot[1:])) == 6, n_hot    # every column holds >= 1 >= th seeds
    n_edge = {d: len(run("main", **dict(BASE, min_edge_distance=d))) for d in EDGE_DISTANCES}
    assert len({n_edge[d] for d in range(8)}) == 8, n_edge
    assert n_edge[2.5] == n_edge[3] != n_edge[2] and n_edge[13] == 0, n_edge       # 13 > Z / 2: no plane is left
    for b in BACK_WIDTHS:
        n = len(run("main", **dict(BASE, background_gfilt_size=b, th_seed=BACK_OFF_TH if b < 0.75 else 500)))
        assert n >= 50, (dtype, b, n)
    n = len(run("noise", **dict(BASE, filt_size=2, gfilt_size=0, th_seed=-1e3)))
    assert n > FIN_CAP, (dtype, n)
