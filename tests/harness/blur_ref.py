"""NumPy restatement of the box-blur normalisation of fft_align.hip (``ia3_blurnorm2d``).

``box_blur(im, gb)`` states what ``cv2.blur(im.astype(np.float32), (gb, gb))`` is taken to be: a normalised
``gb x gb`` box anchored at ``gb // 2`` in both axes, BORDER_REFLECT_101, every window summed in float64 — each
of its rows left to right, then the row sums top to bottom — times the double ``1 / gb**2``, rounded to float32.
OpenCV itself is not installed where this project is built and tested; this file is the pin.  The fixture
generator (scripts/make_fftblur_golden.py) hands ``box_blur`` to the reference as its ``cv2.blur``.
"""
import numpy as np

DIVIDE, SUBTRACT = 0, 1


def reflect101(idx, n):
    """BORDER_REFLECT_101 index: -1 -> 1, -2 -> 2, n -> n - 2, periodic with 2 (n - 1); a length-1 axis is all 0."""
    idx = np.asarray(idx, dtype=np.int64)
    if n == 1:
        return np.zeros_like(idx)
    p = 2 * (n - 1)
    m = np.mod(idx, p)
    return np.where(m < n, m, p - m)


def box_blur(im, gb):
    im = np.asarray(im)
    if im.ndim != 2 or im.dtype != np.float32:
        raise TypeError("box_blur takes a 2-D float32 image")
    gb = int(gb)
    sx, sy = im.shape
    a = gb // 2
    rows = reflect101(np.arange(-a, sx - a + gb - 1), sx)
    cols = reflect101(np.arange(-a, sy - a + gb - 1), sy)
    padded = im[np.ix_(rows, cols)].astype(np.float64)
    row_sums = np.zeros((sx + gb - 1, sy), dtype=np.float64)
    for v in range(gb):                      # each window row, left to right
        row_sums = row_sums + padded[:, v:v + sy]
    total = np.zeros((sx, sy), dtype=np.float64)
    for u in range(gb):                      # the row sums, top to bottom
        total = total + row_sums[u:u + sx]
    return (total * (1.0 / (gb * gb))).astype(np.float32)


def cv2_blur(im, ksize):
    """Stand-in for ``cv2.blur(im, (gb, gb))`` (square boxes only)."""
    if ksize[0] != ksize[1]:
        raise NotImplementedError("square boxes only")
    return box_blur(im, ksize[0])


def blurnorm2d(im, gb, mode):
    im_ = np.asarray(im).astype(np.float32)
    blurred = box_blur(im_, gb)
    with np.errstate(divide="ignore", invalid="ignore"):
        return im_ - blurred if mode == SUBTRACT else im_ / blurred


def bead_blob_pair(dtype):
    """The 20 x 112 x 96 bead pair of tests/golden/fftblur.npz: beads that drift by (1.3, -4.6, 7.25) over a broad
    stationary blob, which decides the unblurred correlation.  Returns (ref, src) quantised to ``dtype``."""
    from imageanalysis3_amd import synth
    shape = (20, 112, 96)
    ref, src, _, _ = synth.make_bead_pair(shape, 10, 21, (1.3, -4.6, 7.25), dtype=np.float64, margin=(6, 14, 14), min_sep=12.0)
    z, x, y = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    blob = 6000.0 * np.exp(-((z - 9) ** 2 / (2 * 6.0 ** 2) + (x - 50) ** 2 / (2 * 30.0 ** 2) + (y - 40) ** 2 / (2 * 25.0 ** 2)))
    return synth.quantise(ref + blob, dtype), synth.quantise(src + blob, dtype)
