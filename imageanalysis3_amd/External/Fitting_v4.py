"""Drop-in for the hot-path part of the reference's ``External/Fitting_v4.py``:
``iter_fit_seed_points`` (:559-683) backed by the wave-per-ball LM kernels of libia3.so.

The class keeps the reference's constructor, ``firstfit()`` / ``repeatfit()`` and the attributes
callers read: ``ps``, ``centers_fit``, ``success``, ``n_iter``, ``centers``, and the four views of a fit — ``gparms``
(per seed ``[im_, X, center]`` of its first fit), ``ims_rec`` (per seed the fitted Gaussian over its ball, or NaN),
``im_subtr`` and ``im_add`` (the float64 image minus the first-fit / the current reconstructions).  The device path
never materialises the views while it fits (fit.hip header); they are rendered on first access by kernels of their own
from the per-seed records the fit left behind, cached on the object, and dropped by the next ``firstfit()`` /
``repeatfit()``.  ``im_add`` is defined per voxel as the image minus the reconstructions that cover it in ascending seed
order, which the reference's in-place updates equal up to float64 rounding order.
``residual_stack()`` gives the same residual as a float32 ``DeviceStack`` for a second seeding pass on the device.  The
fitter handle stays alive for this until the object is deleted or ``release()`` is called; a ``DeviceStack`` passed as
``im`` must stay alive as long (a view asked for after it was freed raises ``AttributeError``).

The module's 2-D FFT aligners are here as well (:733-820, :422-424): ``blurnorm2d`` (the box blur is
*subtracted* here, divided in ``alignment_tools``), ``fftalign_2d`` / ``fft3d_from2d`` with this module's
offset convention (``[y, x] - im2.shape + 1``), its defaults and ``return_cor``, all on the device through
the entries ``alignment_tools`` uses (fft_align.hip), and the small host helpers ``minmax``, ``translate``
and ``closest_faster``.  ``plt_val=True`` (matplotlib figures) is not provided.

The module's fast path is here too (fastfit.hip): ``normalzie_im`` (:94-98), ``get_seed_points_base_v2`` (:100-126),
``gfit_fast`` (:433-490) and ``fast_fit_big_image`` (:496-558) — closed-form moment fits, one wavefront per seed, no LM
and no refit sweeps.  The path is meant for float stacks: on uint16 the reference's ``weights = im_ - bk`` wraps
(``weights < 0`` never holds, heights near 65535 come out), and that is reproduced as it is.  ``get_seed_points_base``
(v1, pyfftw Gaussian), ``troubleshoot=True`` and ``plt_val=True`` are not provided.
"""
import ctypes as C
import numpy as np

from .. import _lib as L
from .. import alignment_tools as _at


def in_dim(x, y, z, xmax, ymax, zmax):
    """External/Fitting_v4.py:399-401."""
    keep = ((x >= 0) & (x < xmax) & (y >= 0) & (y < ymax) & (z >= 0) & (z < zmax)) > 0
    return x[keep], y[keep], z[keep]


def closest_faster(xyz, ic, tree, rsearch=6):
    """External/Fitting_v4.py:422-424 — the columns (3, m) of the rows of ``xyz`` whose nearest point of ``tree`` (the
    caller's ``scipy.spatial.cKDTree``, searched up to ``rsearch``) is point number ``ic``."""
    _, nearest = tree.query(xyz, distance_upper_bound=rsearch)
    return xyz[nearest == ic].T


def blurnorm2d(im, gb):
    """External/Fitting_v4.py:733-737 — the image minus its ``gb x gb`` box blur (float32), on the device."""
    return _at._blurnorm2d(im, gb, L.BLUR_SUBTRACT)


def fft3d_from2d(im1, im2, gb=5, max_disp=150, plt_val=False, return_cor=False):
    """External/Fitting_v4.py:738-752 — integer [tz, tx, ty] from the blur-subtracted z- and then y-max-projections
    (with the two correlation values if ``return_cor``); ndarrays or DeviceStacks, everything on the device."""
    if plt_val:
        raise NotImplementedError("plt_val=True (matplotlib figures) is not provided")
    return _at._fft3d_from2d(im1, im2, gb, L.BLUR_SUBTRACT, L.OFFSET_FITTING_V4, max_disp, return_cor)


def fftalign_2d(im1, im2, center=[0, 0], max_disp=50, plt_val=False, return_cor=False):
    """External/Fitting_v4.py:754-807 — (xt, yt) of the windowed peak of the normalised cross-correlation, counted from
    ``im2``'s far corner (``[y, x] - im2.shape + 1``); with ``return_cor`` also the peak over the smaller image's size."""
    if plt_val:
        raise NotImplementedError("plt_val=True (matplotlib figures) is not provided")
    return _at._fftalign_2d(im1, im2, center, max_disp, L.OFFSET_FITTING_V4, return_cor)


def minmax(im, min_=None, max_=None):
    """External/Fitting_v4.py:808-811 — float32 image rescaled so that [min_, max_] (default: its own range) is [0, 1]."""
    lo = np.min(im) if min_ is None else min_
    hi = np.max(im) if max_ is None else max_
    return (np.array(im, dtype=np.float32) - lo) / (hi - lo)


def translate(im, trans):
    """External/Fitting_v4.py:812-820 — N-D image moved by the rounded ``-trans`` (``out[i] = im[i + t]``); what moves
    in from outside is the image's median (an integer image comes back as float64, as ``zeros + median`` does)."""
    im = np.asarray(im)
    t = np.array(np.round(trans), dtype=int)
    fill = np.median(im)
    out = np.empty(im.shape, dtype=(np.zeros(1, dtype=im.dtype) + fill).dtype)
    out[...] = fill
    src = tuple(slice(max(k, 0), min(n, n + k)) for k, n in zip(t, im.shape))
    dst = tuple(slice(max(-k, 0), min(n, n - k)) for k, n in zip(t, im.shape))
    out[dst] = im[src]
    return out


def _resident(im):
    """(DeviceStack, owned) for an ndarray or a DeviceStack."""
    if isinstance(im, L.DeviceStack):
        return im, False
    return L.DeviceStack.upload(im), True


def _normalise_dev(stack, sz):
    sz = int(sz)
    if sz > L.BLUR_MAX_GB:
        raise NotImplementedError("box size %d: boxes up to %d are supported" % (sz, L.BLUR_MAX_GB))
    h = C.c_void_p()
    L.check(L.lib().ia3_fastfit_normalize_dev(stack._h, sz, C.byref(h)))
    return L.DeviceStack(h, stack.shape, np.float32)


def normalzie_im(im, sz=20):
    """External/Fitting_v4.py:94-98 — ``float32(im)`` minus its ``sz x sz`` box blur, plane by plane, on the device with
    the rules of ``blurnorm2d`` (anchor ``sz // 2``, BORDER_REFLECT_101, float64 window sums; boxes up to 32).  An ndarray
    gives an ndarray, a ``DeviceStack`` a new ``DeviceStack``."""
    stack, owned = _resident(im)
    try:
        out = _normalise_dev(stack, sz)
    finally:
        if owned:
            stack.free()
    if owned:
        with out:
            return out.download()
    return out


def get_seed_points_base_v2(im_sm, gfilt_size=5, filt_size=3, th_seed=3., max_num=None):
    """External/Fitting_v4.py:100-126 — local maxima of the box-normalised stack (``gfilt_size=0``: of the stack as it
    is) above ``th_seed`` times its standard deviation, neighbours within ``int(filt_size/2)`` taken modulo the shape
    (at most 3).  Returns ``(centers_zxyh, std_)``: a (4, N) array [z, x, y, h], brightest first (float64 for a float
    stack, int64 for uint16), and ``np.std`` of the stack — float32 for a float32 stack (the device sums in float64 and
    rounds, NumPy sums in float32: equal to float32 rounding), float64 for uint16."""
    pix = int(filt_size / 2)
    if pix > 3:
        raise NotImplementedError("filt_size %s: neighbours within %d voxels, at most 3 are supported" % (filt_size, pix))
    if int(gfilt_size) != gfilt_size or gfilt_size < 0:
        raise ValueError("gfilt_size is a box size: a non-negative integer")
    if int(gfilt_size) > L.BLUR_MAX_GB:
        raise NotImplementedError("box size %d: boxes up to %d are supported" % (gfilt_size, L.BLUR_MAX_GB))
    stack, owned = _resident(im_sm)
    try:
        is_f32 = int(gfilt_size) != 0 or stack.dtype == np.float32
        strong64 = isinstance(th_seed, np.floating) and np.dtype(type(th_seed)).itemsize >= 8
        cut = -1 if (max_num is None or max_num < 0) else int(max_num)
        capacity, n, sd = 4096, C.c_int(0), C.c_double(0)
        while True:
            rows = np.empty((capacity, 4), dtype=np.float64)
            rc = L.lib().ia3_fastfit_seeds_dev(stack._h, int(gfilt_size), 2 * pix, float(th_seed),
                                               0 if strong64 else 1, cut, L.dptr(rows), capacity, C.byref(n), C.byref(sd))
            if rc == L.IA3_ECAPACITY and n.value > capacity:
                capacity = n.value
                continue
            L.check(rc)
            break
    finally:
        if owned:
            stack.free()
    centers_zxyh = np.ascontiguousarray(rows[:n.value].T)
    if not is_f32:
        centers_zxyh = centers_zxyh.astype(np.int64)
    if max_num is not None and max_num < 0:
        centers_zxyh = centers_zxyh[:, :max_num]
    return centers_zxyh, (np.float32(sd.value) if is_f32 else np.float64(sd.value))


def inv_sigma(sigma):
    """External/Fitting_v4.py:426-432 — inverse of a symmetric 3 x 3 matrix by cofactors."""
    [[a, d, e], [d, b, f], [e, f, c]] = sigma
    det = a * b * c - c * d ** 2 - b * e ** 2 + 2 * d * e * f - a * f ** 2
    return np.array([[(b * c - f ** 2) / det, (-(c * d) + e * f) / det, (-(b * e) + d * f) / det],
                     [(-(c * d) + e * f) / det, (a * c - e ** 2) / det, (d * e - a * f) / det],
                     [(-(b * e) + d * f) / det, (d * e - a * f) / det, (a * b - d ** 2) / det]])


_FAST_KINDS = {np.dtype(np.float32): 0, np.dtype(np.uint16): 1, np.dtype(np.float64): 2}


def gfit_fast(im_, X_, bk_f=0.1, reconstruct=False, plt_val=False, compare_with_fitting=False):
    """External/Fitting_v4.py:433-490 — closed-form moment fit of one voxel set on the device: ``[h, z, x, y, bk, a, b, c,
    d, e, f, eps]`` as float64 (order-statistic background, height, weighted centroid, weighted covariance).  ``im_``:
    (n,) float32, float64 or uint16 values, n <= 512; ``X_``: (3, n) integer coordinates.  ``reconstruct=True`` evaluates
    ``inv_sigma``, the model and ``eps`` on the host from the device's numbers; otherwise ``eps`` is NaN."""
    if plt_val:
        raise NotImplementedError("plt_val=True (matplotlib figures) is not provided")
    im_ = np.asarray(im_)
    if len(im_) == 0:
        return np.array([np.nan] * 12)
    if im_.dtype not in _FAST_KINDS:
        raise TypeError("gfit_fast takes float32, float64 or uint16 values, got %s" % im_.dtype)
    X = np.asarray(X_)
    if X.shape != (3, len(im_)) or X.dtype.kind not in "iu":
        raise ValueError("X_ should be a (3, n) integer array")
    vals = np.ascontiguousarray(im_, dtype=np.float64)
    coords = np.ascontiguousarray(X.T, dtype=np.int32)
    out = np.empty(12, dtype=np.float64)
    L.check(L.lib().ia3_fastfit_voxels(L.dptr(vals), L.ptr(coords), len(vals), _FAST_KINDS[im_.dtype],
                                       float(bk_f), L.dptr(out)))
    if reconstruct:
        h, bk = out[0], out[4]
        a, b, c, d, e, f = out[5:11]
        X_c = X.T - out[1:4]
        iCov = inv_sigma([[a, d, e], [d, b, f], [e, f, c]])
        im_fit = h * np.exp(-np.sum(np.dot(X_c, iCov) * X_c, -1) * 0.5) + bk
        out[11] = np.mean(np.abs(im_ - im_fit))
    return out


def fast_fit_big_image(im, centers_zxy, radius_fit=4, avoid_neigbors=True, recenter=False, verbose=True,
                       better_fit=False, troubleshoot=False):
    """External/Fitting_v4.py:496-558 — ``gfit_fast`` for every centre on the integer ball of ``radius_fit`` (offsets in
    ``[-r, r)``, 254 voxels for 4; at most 5), clipped to the image: (N, 12) float64 rows, shape (0,) for no centres.
    ``avoid_neigbors``: each ball keeps the offsets nearer to its centre than to any other centre within ``2 r`` (ties to
    the lowest index); ``recenter``: the ball moves to its first maximum; ``better_fit``: the LM fit
    ``GaussianFit(delta_center=2.5)`` on the same voxels instead, (N, 11) float32 rows.  ``verbose`` prints nothing.
    ``im``: ndarray or ``DeviceStack``."""
    if troubleshoot:
        raise NotImplementedError("troubleshoot=True (matplotlib figures) is not provided")
    if len(centers_zxy) == 0:
        return np.array([])
    cen = np.ascontiguousarray(centers_zxy, dtype=np.float64)
    if cen.ndim != 2 or cen.shape[1] != 3:
        raise ValueError("centers_zxy should be an (N, 3) array")
    r = int(radius_fit)
    n = len(cen)
    g = np.arange(-r, r)
    nball = int(np.count_nonzero(np.add.outer(np.add.outer(g * g, g * g), g * g) <= r * r))
    if nball > 512:
        raise NotImplementedError("radius_fit %d: balls of up to 512 voxels (radius_fit <= 5) are supported" % r)
    stack, owned = _resident(im)
    try:
        out = np.empty((n, 12), dtype=np.float64)
        if better_fit:
            cnt = np.empty(n, dtype=np.int32)
            vals = np.empty((n, nball), dtype=np.float64)
            zxy = np.empty((n, nball, 3), dtype=np.int32)
            extra = (L.ptr(cnt), L.dptr(vals), L.ptr(zxy))
        else:
            extra = (None, None, None)
        L.check(L.lib().ia3_fastfit_moments_dev(stack._h, L.dptr(cen), n, r, 1 if avoid_neigbors else 0,
                                                1 if recenter else 0, 0.1, L.dptr(out), *extra))
        dtype = stack.dtype
    finally:
        if owned:
            stack.free()
    if not better_fit:
        return out
    ps = np.full((n, 11), np.nan, dtype=np.float32)
    rows = [i for i in range(n) if cnt[i] > 0]
    ims = [vals[i, :cnt[i]].astype(dtype) for i in rows]
    Xs = [zxy[i, :cnt[i]].T for i in rows]
    starts = [X[:, np.argmax(v)] for v, X in zip(ims, Xs)]       # the voxel of the ball's first maximum
    big = [k for k, v in enumerate(ims) if len(v) >= 10]         # GaussianFit.fit leaves fewer voxels unfitted (:382-383)
    if big:
        fitted = gaussfit_batch([ims[k] for k in big], [Xs[k] for k in big], [starts[k] for k in big], delta_center=2.5)[0]
        for k, row in zip(big, fitted):
            ps[rows[k]] = row
    for k in set(range(len(rows))) - set(big):
        ps[rows[k]] = GaussianFit(ims[k], Xs[k], center=starts[k], delta_center=2.5).p
    return ps


def gaussfit_batch(ims, Xs, centers, delta_center=3., min_w=0.5, max_w=4., init_w=1.5):
    """Run many independent ``GaussianFit(im, X, center=...).fit()`` in one launch (one wave per fit).
    ims: list of 1-D voxel-value arrays; Xs: list of (3,n) coordinate arrays; centers: (N,3).
    Returns (ps (N,11) float32, xs (N,10) float64, success (N,) bool, nfev (N,) int)."""
    n_fits = len(ims)
    off = np.zeros(n_fits + 1, dtype=np.int32)
    kinds = np.zeros(n_fits, dtype=np.int32)
    for i, im in enumerate(ims):
        im = np.asarray(im)
        off[i + 1] = off[i] + im.size
        kinds[i] = 1 if im.dtype.kind in "ui" else (0 if im.dtype == np.float32 else 2)
    vals = np.concatenate([np.asarray(im, dtype=np.float64).ravel() for im in ims]) if n_fits else np.zeros(0)
    coords = (np.concatenate([np.asarray(X).T.reshape(-1, 3) for X in Xs]).astype(np.int32)
              if n_fits else np.zeros((0, 3), np.int32))
    vals, coords = np.ascontiguousarray(vals), np.ascontiguousarray(coords)
    cen = np.ascontiguousarray(np.asarray(centers, dtype=np.float64).reshape(n_fits, 3))
    cfg = np.ascontiguousarray(np.tile(np.array([delta_center, min_w, max_w, init_w], dtype=np.float64), (n_fits, 1)))
    ps = np.full((n_fits, 11), np.nan, dtype=np.float32)
    xs = np.full((n_fits, 10), np.nan, dtype=np.float64)
    info = np.zeros((n_fits, 2), dtype=np.int32)
    L.check(L.lib().ia3_gaussfit_voxels(L.dptr(vals), L.ptr(coords), L.ptr(off), n_fits, L.dptr(cen), L.dptr(cfg),
                                        L.ptr(kinds), L.ptr(ps), L.dptr(xs), L.ptr(info)))
    return ps, xs, info[:, 0].astype(bool), info[:, 1]


class GaussianFit():
    """External/Fitting_v4.py:165-396 — one constrained 10-parameter 3-D Gaussian fit on an explicit voxel
    list.  ``fit()`` runs the wave-per-fit LM kernel (ia3_gaussfit_voxels); the small helpers below
    (``to_natural_paramaters``, ``get_im``) evaluate the closed-form model on the host for the <= 512
    voxels of one fit, as the reference does."""

    def __init__(self, im, X, center=None, n_aprox=10, min_w=0.5, max_w=4., delta_center=3.,
                 init_w=1.5):
        self._min_w, self._max_w, self._init_w = min_w, max_w, init_w
        self.min_w = min_w * min_w
        self.max_w = max_w * max_w
        self.delta_center = delta_center
        self._im_in = np.asarray(im)
        self._X_in = np.asarray(X)
        self.im = np.array(im, dtype=np.float32)
        self.x, self.y, self.z = np.array(X, dtype=np.float32)
        argsort_im = np.argsort(im)
        if center is None:                                                        # :176-177
            center = np.median(self._X_in[:, argsort_im][:, -n_aprox:], -1)
        self.center_est = center
        if n_aprox != 10:
            raise NotImplementedError("n_aprox != 10")
        sorted_im = self._im_in[argsort_im]
        eps = np.exp(-10.)
        bk_guess = np.log(np.max([np.mean(sorted_im[:n_aprox]), eps]))
        h_guess = np.log(np.max([np.mean(sorted_im[-n_aprox:]), eps]))
        wsq = init_w ** 2
        wg = np.log((self.max_w - wsq) / (wsq - self.min_w))
        self.p_ = np.array([bk_guess, h_guess, 0, 0, 0, wg, wg, wg, 0, 0], dtype=np.float32)
        self.to_natural_paramaters()
        self.success = False

    # -- closed-form model on the host (Fitting_v4.py:189-290) ---------------------------------
    def _sig(self, v, lo, hi):
        v = np.float64(v)
        lim = np.log(np.finfo(np.float64).max)
        if v >= lim:
            return lo
        if v <= -lim:
            return hi
        return (hi - lo) / (1. + np.exp(v)) + lo

    def _geom(self, parms):
        bk, h, xp, yp, zp, w1, w2, w3, pp, tp = [np.float64(v) for v in parms]
        t, p = self._sig(tp, -1., 1.), self._sig(pp, -1., 1.)
        ws = [self._sig(w, self.min_w, self.max_w) for w in (w1, w2, w3)]
        d = self.delta_center
        c = [self._sig(v, -d, d) + np.float64(c0) for v, c0 in zip((xp, yp, zp), self.center_est)]
        return bk, h, t, p, ws, c

    def calc_f(self, parms):
        self.p_ = parms
        bk, h, t, p, (ws1, ws2, ws3), (xc, yc, zc) = self._geom(parms)
        xt, yt, zt = self.x - xc, self.y - yc, self.z - zc
        p2, t2 = p * p, t * t
        tc2, pc2 = 1 - t2, 1 - p2
        tc, pc = np.sqrt(tc2), np.sqrt(pc2)
        s1, s2, s3 = 1. / ws1, 1. / ws2, 1. / ws3
        x2c = pc2 * tc2 * s1 + t2 * s2 + p2 * tc2 * s3
        y2c = pc2 * t2 * s1 + tc2 * s2 + p2 * t2 * s3
        z2c = p2 * s1 + pc2 * s3
        xyc = 2 * tc * t * (pc2 * s1 - s2 + p2 * s3)
        xzc = 2 * p * pc * tc * (s3 - s1)
        yzc = 2 * p * pc * t * (s3 - s1)
        xsigmax = x2c * xt * xt + y2c * yt * yt + z2c * zt * zt + xyc * xt * yt + xzc * xt * zt + yzc * yt * zt
        self.f0 = np.exp(h - 0.5 * xsigmax)
        self.f = np.exp(np.clip(bk, -709.78, 709.78)) + self.f0
        return self.f

    def calc_eps(self, parms):
        return self.calc_f(parms) - self.im

    def to_natural_paramaters(self, parms=None):
        if parms is None:
            parms = self.p_
        bk, h, t, p, ws, c = self._geom(parms)
        eps = np.mean(np.abs(self.calc_eps(parms)))
        self.p = np.array([np.exp(h), c[0], c[1], c[2], np.exp(bk), np.sqrt(ws[0]), np.sqrt(ws[1]), np.sqrt(ws[2]),
                           t, p, eps], dtype=np.float32)
        return self.p

    def fit(self, eps_frac=10E-3, eps_dist=10E-3, eps_angle=10E-3):
        """Levenberg-Marquardt on the device; results in ``self.p`` = [height, c0, c1, c2, background,
        width_0, width_1, width_2, sin_theta, sin_phi, error] (Fitting_v4.py:377-393)."""
        if len(self.p_) > len(self.im):
            self.success = False
        else:
            ps, xs, ok, nfev = gaussfit_batch([self._im_in], [self._X_in], [self.center_est],
                                              delta_center=self.delta_center, min_w=self._min_w,
                                              max_w=self._max_w, init_w=self._init_w)
            self.p_ = xs[0]
            self.p = ps[0]
            self.center = self.p[1:4]
            self.nfev = int(nfev[0])
            self.success = True

    def get_im(self):
        self.calc_f(self.p_)
        return self.f0


def split_voxel_sets(counts, zxy, vals, centers, dtype):
    """The reference's ``gparms`` from the packed buffers of ``ia3_fit_view_voxels``: per seed ``[im_, X, center]`` with
    ``im_`` the first ``counts[i]`` values in the image's dtype, ``X`` their (3, nvox) int64 coordinates and ``center``
    the seed as a list."""
    dtype = np.dtype(dtype)
    return [[vals[i, :k].astype(dtype), np.ascontiguousarray(zxy[i, :k].T, dtype=np.int64), [float(v) for v in centers[i]]]
            for i, k in enumerate(int(c) for c in counts)]


def split_reconstructions(counts, has_rec, recs):
    """The reference's ``ims_rec`` from the packed buffers of ``ia3_fit_view_recs``: per seed a float64 array of
    ``counts[i]`` values, or the scalar ``np.nan`` where no fit of the seed has succeeded."""
    return [np.array(recs[i, :int(k)], dtype=np.float64) if h else np.nan for i, (k, h) in enumerate(zip(counts, has_rec))]


class iter_fit_seed_points():
    def __init__(self, im, centers, radius_fit=5, min_delta_center=1., max_delta_center=2.5,
                 n_max_iter=10, max_dist_th=0.1,
                 min_w=0.5, max_w=4, init_w=1.5):
        """``im``: (z,x,y) ndarray (uint16/float32) or a DeviceStack; ``centers``: (3,N) like the
        reference (it stores ``centers.T``)."""
        self.im = im
        self.radius_fit = radius_fit
        self.n_max_iter = n_max_iter
        self.max_dist_th = max_dist_th
        self.min_delta_center = min_delta_center
        self.max_delta_center = max_delta_center
        centers = np.asarray(centers, dtype=np.float64)
        self.centers = centers.T if centers.size else np.zeros((0, 3))
        if self.centers.ndim != 2 or (len(self.centers) and self.centers.shape[1] != 3):
            raise IndexError("centers should be a (3, N) array")
        self.z, self.x, self.y = (self.centers[:, 0], self.centers[:, 1], self.centers[:, 2])
        self.zb, self.xb, self.yb = np.reshape(np.indices([self.radius_fit * 2] * 3) - self.radius_fit, [3, -1])
        keep = self.zb * self.zb + self.xb * self.xb + self.yb * self.yb <= self.radius_fit ** 2
        self.zb, self.xb, self.yb = self.zb[keep], self.xb[keep], self.yb[keep]
        self.zxyb = np.array([self.zb, self.xb, self.yb]).T
        self.sz, self.sx, self.sy = im.shape
        self.min_w = min_w
        self.max_w = max_w
        self.init_w = init_w
        self._own_stack = None
        self._fitter = None
        self._fitted = False      # firstfit() has run on at least one seed: the views exist
        self.keep_views = True    # False before firstfit(): no first-fit snapshot is kept and the views are not offered
        self.ps = []
        self.success = []
        self.centers_fit = []
        self.n_iter = 0

    # -- device plumbing ---------------------------------------------------------------------
    def _ensure(self):
        if self._fitter is not None:
            return
        if isinstance(self.im, L.DeviceStack):
            stack = self.im
        else:
            self._own_stack = L.DeviceStack.upload(self.im)
            stack = self._own_stack
        self._stack = stack
        p = self._fit_params()
        c = np.ascontiguousarray(self.centers, dtype=np.float64)
        h = C.c_void_p()
        L.check(L.lib().ia3_fit_create(stack._h, L.dptr(c), len(c), C.byref(p), C.byref(h)))
        self._fitter = h

    def _fit_params(self):
        return L.make_fit_params(self.radius_fit, self.min_delta_center, self.max_delta_center, self.n_max_iter,
                                 self.max_dist_th, self.min_w, self.max_w, self.init_w)

    def _pull(self):
        n = len(self.centers)
        ps = np.empty((n, 11), dtype=np.float32)
        ok = np.empty(n, dtype=np.uint8)
        nv = np.empty(n, dtype=np.int32)
        L.check(L.lib().ia3_fit_results(self._fitter, L.ptr(ps), L.ptr(ok), L.ptr(nv)))
        self.ps = [ps[i] for i in range(n)]
        self.success = [bool(v) for v in ok]
        self.centers_fit = [ps[i, 1:4] for i in range(n)]
        self.nvox = nv

    def release(self):
        """Give the fitter handle and the uploaded copy of a host image back.  ``ps``, ``success`` and every view
        that has been read stay; a view that has not been rendered yet is gone."""
        if self._fitter is not None:
            L.lib().ia3_fit_destroy(self._fitter)
            self._fitter = None
        if self._own_stack is not None:
            self._own_stack.free()
            self._own_stack = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass

    # -- views of the fit (External/Fitting_v4.py:597-598, :605, :623, :632-639, :674-675) ------------------------
    _VIEWS = ("gparms", "ims_rec", "im_subtr", "im_add")

    def _drop_views(self):
        for name in self._VIEWS:
            self.__dict__.pop(name, None)

    def __getattr__(self, name):   # reached only for names the object does not hold
        if name not in iter_fit_seed_points._VIEWS:
            raise AttributeError("%r object has no attribute %r" % (type(self).__name__, name))
        if not self.__dict__.get("_fitted"):   # before firstfit(), or no seeds: the reference has not made them either
            raise AttributeError("%r object has no attribute %r (firstfit() has not fitted any seed)"
                                 % (type(self).__name__, name))
        if not self.keep_views:
            raise AttributeError("%s was not kept: keep_views was False at firstfit()" % name)
        if self._fitter is None:
            raise AttributeError("%s was not rendered before the fitter was released (release())" % name)
        self._check_stack()
        value = getattr(self, "_render_" + name)()
        self.__dict__[name] = value
        return value

    def _check_stack(self):
        """A ``DeviceStack`` passed as ``im`` belongs to the caller and has to outlive the views: the kernels read it."""
        if self._stack._h is None:
            raise AttributeError("the DeviceStack this fitter reads has been freed: views are rendered from the image")

    def _render_gparms(self):
        n, nball = len(self.centers), len(self.zb)
        cnt = np.empty(n, dtype=np.int32)
        zxy = np.empty((n, nball, 3), dtype=np.int32)
        vals = np.empty((n, nball), dtype=np.float64)
        L.check(L.lib().ia3_fit_view_voxels(self._fitter, L.ptr(cnt), L.ptr(zxy), L.dptr(vals)))
        return split_voxel_sets(cnt, zxy, vals, self.centers, self._stack.dtype)

    def _records(self, which=1):
        """(counts, has_rec, recs (n, nball), x11 (n, 11)) of the first-fit (0) or the current (1) records; the rows of
        ``x11`` are the unconstrained parameters of ``GaussianFit.p_`` and the ``delta_center`` of that fit."""
        n, nball = len(self.centers), len(self.zb)
        cnt = np.empty(n, dtype=np.int32)
        has = np.empty(n, dtype=np.uint8)
        recs = np.empty((n, nball), dtype=np.float64)
        x11 = np.empty((n, 11), dtype=np.float64)
        L.check(L.lib().ia3_fit_view_recs(self._fitter, int(which), L.ptr(cnt), L.ptr(has), L.dptr(recs), L.dptr(x11)))
        return cnt, has, recs, x11

    def _render_ims_rec(self):
        cnt, has, recs, _ = self._records(1)
        return split_reconstructions(cnt, has, recs)

    def _render_residual(self, which):
        out = np.empty((self.sz, self.sx, self.sy), dtype=np.float64)
        L.check(L.lib().ia3_fit_view_residual(self._fitter, which, L.dptr(out)))
        return out

    def _render_im_subtr(self):
        return self._render_residual(0)

    def _render_im_add(self):
        return self._render_residual(1)

    def residual_stack(self, which="add"):
        """``im_subtr`` (``"subtr"``) or ``im_add`` (``"add"``) rounded once to float32, as a new ``DeviceStack``:
        ``get_seeds`` / ``fit_fov_image`` take it as it is, so a second pass on the residual never leaves the device."""
        if which not in ("subtr", "add"):
            raise ValueError("which should be 'subtr' or 'add'")
        if not self._fitted or not self.keep_views:
            raise AttributeError("no residual: firstfit() has not fitted any seed, or keep_views was False")
        if self._fitter is None:
            raise AttributeError("no residual: the fitter was released (release())")
        self._check_stack()
        h = C.c_void_p()
        L.check(L.lib().ia3_fit_view_residual_dev(self._fitter, 0 if which == "subtr" else 1, C.byref(h)))
        return L.DeviceStack(h, (self.sz, self.sx, self.sy), np.float32)

    # -- reference API -----------------------------------------------------------------------
    def firstfit(self):
        """External/Fitting_v4.py:590-639 — Voronoi-restricted first fit of every seed."""
        if len(self.centers) > 0:
            self._ensure()
            self._drop_views()
            L.check(L.lib().ia3_fit_first(self._fitter))
            if self.keep_views:
                L.check(L.lib().ia3_fit_snapshot(self._fitter))   # im_subtr is made from these records later
            self._fitted = True
            self._pull()

    def repeatfit(self):
        """External/Fitting_v4.py:641-683 — ordered Gauss-Seidel refit sweeps until converged."""
        self.n_iter = 0
        self.converged = np.zeros(len(self.centers), dtype=bool)
        if len(self.centers) > 0:
            if self._fitter is None:
                raise AttributeError("repeatfit() called before firstfit()")
            n_iter = C.c_int(0)
            self._drop_views()
            L.check(L.lib().ia3_fit_repeat(self._fitter, C.byref(n_iter)))
            self.n_iter = int(n_iter.value)
            self._pull()
            self.converged[:] = True

    def stats(self):
        """(number of LM fits run, total function evaluations) so far — for the flop accounting."""
        a, b = C.c_int64(0), C.c_int64(0)
        L.check(L.lib().ia3_fit_stats(self._fitter, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)
