"""NumPy statement of the residual images the fitter's views render (fit.hip, "Views of a finished fit").

The residual of a fit is defined per voxel: start from ``float64(im)`` and subtract, in ascending seed index, the
reconstruction of every seed that has one and whose ball holds the voxel — ``((im - rec_a) - rec_b) - ...``.  The device
forms that chain in the wave of the voxel's OWNER, the lowest seed whose ball holds it (with or without a
reconstruction); ``residual`` below walks the seeds instead, which gives every voxel the same chain.  tests/
test_fit_views_cpu.py holds the statement to the oracle's ``im_subtr`` bit for bit and to its ``im_add`` within
rounding order.
"""
import numpy as np


def ball_offsets(radius):
    """Offsets (zb, xb, yb) of the integer ball, ``np.indices`` order (External/Fitting_v4.py:580-582)."""
    zb, xb, yb = np.reshape(np.indices([radius * 2] * 3) - radius, [3, -1])
    keep = zb * zb + xb * xb + yb * yb <= radius ** 2
    return zb[keep], xb[keep], yb[keep]


def ball_voxels(center, radius, shape):
    """(3, m) int64 coordinates of ball ∩ image of one seed, ball order (:607-610)."""
    zb, xb, yb = ball_offsets(radius)
    z, x, y = int(center[0]) + zb, int(center[1]) + xb, int(center[2]) + yb
    keep = (z >= 0) & (z < shape[0]) & (x >= 0) & (x < shape[1]) & (y >= 0) & (y < shape[2])
    return np.array([z[keep], x[keep], y[keep]], dtype=np.int64)


def has_rec(rec):
    """A reconstruction is an array; the reference leaves the scalar NaN where no fit succeeded."""
    return isinstance(rec, np.ndarray) and rec.ndim == 1


def residual(im, centers, ims_rec, radius):
    """float64 image minus the reconstructions, seeds ascending: every voxel gets ((im - rec_a) - rec_b) - ..."""
    out = np.array(im, dtype=np.float64)
    for c, rec in zip(centers, ims_rec):
        if not has_rec(rec):
            continue
        z, x, y = ball_voxels(c, radius, out.shape)
        assert len(rec) == len(z)
        out[z, x, y] = out[z, x, y] - rec     # the voxels of one ball are distinct
    return out


def coverage(shape, centers, radius):
    """(count, owner): per voxel the number of balls that hold it and the lowest seed among them (-1: none)."""
    count = np.zeros(shape, dtype=np.int32)
    owner = np.full(shape, -1, dtype=np.int64)
    for i in range(len(centers) - 1, -1, -1):
        z, x, y = ball_voxels(centers[i], radius, shape)
        count[z, x, y] += 1
        owner[z, x, y] = i
    return count, owner


def residual_by_owner(im, centers, ims_rec, radius):
    """The same residual the way the device organises it: every covered voxel is written once, by its owner, as the
    chain over the seeds that hold it (owner first, then ascending).  Slow; for the CPU test of the two forms."""
    out = np.array(im, dtype=np.float64)
    shape = out.shape
    _, owner = coverage(shape, centers, radius)
    vox = [ball_voxels(c, radius, shape) for c in centers]
    lookup = []
    for X, rec in zip(vox, ims_rec):
        lookup.append(dict(zip(map(tuple, X.T), rec)) if has_rec(rec) else None)
    cen = np.asarray(centers, dtype=np.float64)
    for i, X in enumerate(vox):
        near = [j for j in range(i, len(centers)) if ((cen[j] - cen[i]) ** 2).sum() <= (2.0 * radius) ** 2]
        for v in map(tuple, X.T):
            if owner[v] != i:
                continue
            val = np.float64(im[v])
            for j in near:
                if lookup[j] is not None and v in lookup[j]:
                    val = val - lookup[j][v]
            out[v] = val
    return out


_oracle = {}


def oracle_fit(name, radius=5):
    """The oracle's fit of a committed fixture, made once per process and shared by the tests (do not modify):
    (im, seeds, first, f) — ``first``: copies of what ``firstfit()`` left (ims_rec, im_subtr, im_add, ps, success), ``f``:
    the oracle's object after ``repeatfit()`` (its ``gparms`` are the first fit's)."""
    key = (name, radius)
    if key not in _oracle:
        import np_oracle as O
        from conftest import build_case
        im = build_case(name)
        seeds = O.get_seeds(im, th_seed=600)
        f = O.iter_fit_seed_points(im, seeds.T, radius_fit=radius)
        f.firstfit()
        first = dict(ims_rec=[np.array(r) for r in f.ims_rec], im_subtr=f.im_subtr.copy(), im_add=f.im_add.copy(),
                     ps=np.array(f.ps, dtype=np.float64), success=list(f.success))
        f.repeatfit()
        _oracle[key] = (im, seeds, first, f)
    return _oracle[key]
