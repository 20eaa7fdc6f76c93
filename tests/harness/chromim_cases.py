"""TEST INFRASTRUCTURE — deterministic inputs of the chromosome-image tests (the generator of chromseg_cases): the round
images, their drifts and flags, the images with designed medians, the two small save files of tests/golden/chromim.npz
(scripts/make_chrom_image_golden.py stores the reference's outputs for them, the tests build the inputs again) and the
float64 images of the candidate tests."""
import numpy as np

from . import chromseg_cases as CC

# odd voxel count, Y no multiple of 8 | even count, aligned rows | several blocks, chromseg_cases' "small" shape
SHAPES = {"odd": (5, 19, 37), "even": (6, 32, 64), "small": (12, 40, 72)}
COUNTS = (1, 10, 23)
FLAG2 = (4, 12, 22)                             # rows of drifts() whose image counts as warped
PICK = {1: [7], 10: [0, 4, 7, 8, 10, 11, 13, 16, 19, 20], 23: list(range(23))}


def drifts(shape):
    """23 drifts as a save file holds them (float32): zero, each sign on each axis, all three axes, y shifts that are odd
    and multiples of 8, half-integers (rounded half to even), one plane / row / column of overlap on each axis."""
    Z, X, Y = shape
    d = [(0, 0, 0),
         (1, 0, 0), (-2, 0, 0), (0, 3, 0), (0, -1, 0), (0, 0, 5), (0, 0, -3),
         (1, -2, 3),
         (0, 0, 8), (0, 0, -8), (-1, 2, -7),
         (0.5, 1.5, 2.5), (-0.5, -1.5, 0.5), (2.5, -0.5, -1.5), (1.5, 2.5, -2.5),
         (Z - 1, 0, 0), (1 - Z, 0, 0), (0, X - 1, 0), (0, 1 - X, 0), (0, 0, Y - 1), (0, 0, 1 - Y),
         (Z - 1, 1 - X, Y - 1),
         (0.3, -0.4, 16.2)]
    return np.array(d, dtype=np.float32)


def flags():
    return np.array([2 if k in FLAG2 else 1 for k in range(23)], dtype=np.uint8)


def image(shape, k):
    """Round image k of ``shape``: Poisson(400) background with a few blobs."""
    return CC.stack(shape, 3, 1000 + 37 * k + shape[2], "u16")


def case(name, count):
    """(images, flags, drifts) of ``count`` rounds of shape ``name``."""
    shape, rows = SHAPES[name], PICK[count]
    return [image(shape, k) for k in rows], flags()[rows], drifts(shape)[rows]


SLOW_DRIFTS = np.array([(0.3, -1.7, 2.4), (-0.5, 1.5, 0.25), (0, 0, 0), (1, -2, 3), (0.75, 0.5, -40.5)], dtype=np.float32)
SLOW_FLAGS = np.array([1, 1, 1, 2, 1], dtype=np.uint8)


def slow_case(name):
    """``fast=False``: fractional drifts, one beyond an axis (all cval; set to the axis length + 2.5 here), one warped."""
    shape = SHAPES[name]
    d = SLOW_DRIFTS.copy()
    d[4, 2] = -(shape[2] + 2.5)
    return [image(shape, 40 + k) for k in range(len(d))], SLOW_FLAGS.copy(), d


def median_images(shape):
    """name -> uint16 image: "half" (even counts only: the two middle order statistics are 400 and 401), "equal" (both
    are 400, or the one middle value of an odd count), "constant"."""
    n = int(np.prod(shape))
    rng = np.random.RandomState(n)
    d = {"constant": np.full(shape, 731, np.uint16)}
    lo = np.concatenate([rng.randint(300, 401, size=n // 2 - 1), [400, 400]])   # sorted positions n // 2 - 1 and n // 2
    hi = rng.randint(401, 500, size=n - len(lo))
    d["equal"] = rng.permutation(np.concatenate([lo, hi])).reshape(shape).astype(np.uint16)
    if n % 2 == 0:
        lo = np.concatenate([rng.randint(300, 401, size=n // 2 - 1), [400]])
        hi = np.concatenate([[401], rng.randint(401, 500, size=n // 2 - 1)])
        d["half"] = rng.permutation(np.concatenate([lo, hi])).reshape(shape).astype(np.uint16)
    return d


# ---- save files ----------------------------------------------------------------------------------------------------------------
FILES = {"odd23": ("odd", 23, "unique", 10), "even10": ("even", 10, "combo", 4)}   # shape, rounds, data type, batch


def file_layout(key):
    """(shape, data type, batch, ids, slot of every round): the rounds sit in file order with two empty slots (flag 0)
    among them; ids are not in ascending order."""
    name, count, data_type, batch = FILES[key]
    n = count + 2
    ids = [(7 * k + 3) % 101 + 1 for k in range(n)]
    empty = (2, n - 3)
    slots = [k for k in range(n) if k not in empty]
    return SHAPES[name], data_type, batch, ids, slots


def write_file(B, path, key):
    """The save file ``key`` at ``path`` through ``B`` (classes.batch_functions of the package under test)."""
    name, count, _, _ = FILES[key]
    shape, data_type, _, ids, slots = file_layout(key)
    ims, fl, dr = case(name, count)
    B.create_fov_save_file(path, data_type, ids, ["647"] * len(ids), shape, max_num_seeds=4, overwrite=True)
    for warped in (False, True):
        rows = [k for k in range(count) if (fl[k] == 2) == warped]
        if rows:
            B.save_image_to_fov_file(path, [ims[k] for k in rows], data_type, [ids[slots[k]] for k in rows],
                                     warp_image=warped, drift=[dr[k] for k in rows], verbose=False)
    return ims, fl, dr


# ---- float64 images of the candidate tests --------------------------------------------------------------------------------------
# chromseg_cases' shapes; blob counts, seeds and percentiles chosen so that the statement alone finds at least three
# objects and removes at least one label by size in every case (tests/test_chrom_image_cpu.py asserts it)
CANDIDATES = {"small": dict(shape=CC.STACKS["small"][0], blobs=12, seed=13, percentiles=(97.0, 90.0)),
              "large": dict(shape=CC.STACKS["large"][0], blobs=14, seed=12, percentiles=(98.0, 90.0))}
CAND_FILT_SIZES = (3, 4)
CAND_MIN_SIZE = 100
CAND_NOISE = 60.0


def round_copies(name, n=10):
    """(images, flags, drifts): ``n`` copies of the generated stack ``name``, each moved by a few voxels and with its own
    Gaussian noise; the drift stored with it moves it back, up to a fraction of a voxel."""
    c = CANDIDATES[name]
    base = CC.stack(c["shape"], c["blobs"], c["seed"], "u16").astype(np.int64)
    rng = np.random.RandomState(77 + c["seed"])
    ims, dr = [], []
    for k in range(n):
        d = rng.randint(-2, 3, size=3)
        moved = np.roll(base, tuple(int(v) for v in d), axis=(0, 1, 2))      # moved[j] = base[j - d]
        noise = np.round(rng.normal(0, CAND_NOISE, size=base.shape)).astype(np.int64)
        ims.append(np.clip(moved + noise, 0, 65535).astype(np.uint16))
        dr.append(d + rng.uniform(-0.4, 0.4, size=3))
    return ims, np.ones(n, np.uint8), np.array(dr, dtype=np.float32)


def candidate_cases():
    """(key, stack name, kind, filt_size, percentile): kind "sum" = the chromosome image of round_copies, "seventh" = that
    image divided by 7 (values that are not exact in float32)."""
    out = []
    for name, c in CANDIDATES.items():
        for kind in ("sum", "seventh") if name == "small" else ("sum",):
            for fs in CAND_FILT_SIZES:
                for per in c["percentiles"]:
                    out.append(("%s_%s_f%d_p%g" % (name, kind, fs, per), name, kind, fs, per))
    return out
