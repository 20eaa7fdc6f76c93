"""Drop-in for the hot-path part of the reference's ``alignment_tools.py`` (:278-353):
pixel-level drift from max-projections by FFT cross-correlation, on the device (fft_align.hip).
The underscored helpers carry the mode / offset-convention switches that ``External.Fitting_v4``'s
twins of these functions use."""
import ctypes as C
import numpy as np

from . import _lib as L


def _blurnorm2d(im, gb, mode):
    """OpenCV's normalised ``gb x gb`` box blur of ``im.astype(np.float32)`` and the divide (``BLUR_DIVIDE``) or subtract (``BLUR_SUBTRACT``) that
    follows it, by the box kernel of fft_align.hip (ia3_blurnorm2d: anchor ``gb // 2``, BORDER_REFLECT_101)."""
    a = np.ascontiguousarray(im, dtype=np.float32)
    if a.ndim != 2:
        raise IndexError("blurnorm2d takes a 2-D image")
    out = np.empty_like(a)
    L.check(L.lib().ia3_blurnorm2d(L.ptr(a), a.shape[0], a.shape[1], int(gb), int(mode), L.ptr(out)))
    return out


def blurnorm2d(im, gb):
    """alignment_tools.py:278-283 — the image divided by its ``gb x gb`` box blur (float32), on the device."""
    return _blurnorm2d(im, gb, L.BLUR_DIVIDE)


def _fftalign_2d(im1, im2, center, max_disp, convention, return_cor):
    a = np.ascontiguousarray(im1, dtype=np.float64)
    b = np.ascontiguousarray(im2, dtype=np.float64)
    if a.ndim != 2 or b.ndim != 2:
        raise IndexError("fftalign_2d takes 2-D images")
    c = np.ascontiguousarray(center, dtype=np.float64)
    out = (C.c_int * 2)()
    cor = C.c_double(0.)
    L.check(L.lib().ia3_fftalign_2d_ex(L.dptr(a), a.shape[0], a.shape[1], L.dptr(b), b.shape[0], b.shape[1],
                                       L.dptr(c), float(max_disp), int(convention), out,
                                       C.byref(cor) if return_cor else None))
    return (int(out[0]), int(out[1]), float(cor.value)) if return_cor else (int(out[0]), int(out[1]))


def fftalign_2d(im1, im2, center=[0, 0], max_disp=150, plt_val=False):
    """alignment_tools.py:286-328 — (xt, yt) of the windowed peak of the normalised cross-correlation."""
    a = np.ascontiguousarray(im1, dtype=np.float64)
    b = np.ascontiguousarray(im2, dtype=np.float64)
    if a.ndim != 2 or b.ndim != 2:
        raise IndexError("fftalign_2d takes 2-D images")
    c = np.ascontiguousarray(center, dtype=np.float64)
    out = (C.c_int * 2)()
    L.check(L.lib().ia3_fftalign_2d(L.dptr(a), a.shape[0], a.shape[1], L.dptr(b), b.shape[0], b.shape[1],
                                    L.dptr(c), float(max_disp), out))
    return int(out[0]), int(out[1])


def _fft3d_from2d(im1, im2, gb, mode, convention, max_disp, return_cor):
    """The max-projection chain on the device (ia3_fft3d_from2d(_dev)_ex): projections, their box-blur normalisation
    when ``gb > 1`` and the correlations; ndarrays are uploaded, resident stacks are used where they are."""
    out = (C.c_int * 3)()
    cor = (C.c_double * 2)()
    pc = cor if return_cor else None
    if isinstance(im1, L.DeviceStack) and isinstance(im2, L.DeviceStack):
        L.check(L.lib().ia3_fft3d_from2d_dev_ex(im1._h, im2._h, int(gb), int(mode), int(convention),
                                                float(max_disp), out, pc))
    else:
        a, b = L.as_stack_array(_host(im1)), L.as_stack_array(_host(im2))
        if a.shape != b.shape or a.dtype != b.dtype:
            raise IndexError("fft3d_from2d needs two stacks of the same shape and dtype")
        L.check(L.lib().ia3_fft3d_from2d_ex(L.ptr(a), L.ptr(b), L.dtype_code(a), a.shape[0], a.shape[1], a.shape[2],
                                            int(gb), int(mode), int(convention), float(max_disp), out, pc))
    t = np.array([out[0], out[1], out[2]])
    return (t, float(cor[0]), float(cor[1])) if return_cor else t


def fft3d_from2d(im1, im2, gb=5, max_disp=150):
    """alignment_tools.py:330-353 — integer [tz, tx, ty]; max-projections, their blur normalisation (``gb > 1``) and the
    FFTs on the device.  ``im1``/``im2`` may be ndarrays or DeviceStacks; a resident pair is never downloaded."""
    if gb > 1:
        return _fft3d_from2d(im1, im2, gb, L.BLUR_DIVIDE, L.OFFSET_ALIGNMENT_TOOLS, max_disp, False)
    out = (C.c_int * 3)()
    if isinstance(im1, L.DeviceStack) and isinstance(im2, L.DeviceStack):
        L.check(L.lib().ia3_fft3d_from2d_dev(im1._h, im2._h, float(max_disp), out))
    else:
        a, b = L.as_stack_array(_host(im1)), L.as_stack_array(_host(im2))
        if a.shape != b.shape or a.dtype != b.dtype:
            raise IndexError("fft3d_from2d needs two stacks of the same shape and dtype")
        L.check(L.lib().ia3_fft3d_from2d(L.ptr(a), L.ptr(b), L.dtype_code(a), a.shape[0], a.shape[1], a.shape[2],
                                         float(max_disp), out))
    return np.array([out[0], out[1], out[2]])


def _host(im):
    return im.download() if isinstance(im, L.DeviceStack) else im


def translation_align_pts(cents_fix, cents_target, cutoff=2., xyz_res=1,
                          plt_val=False, return_pts=False, verbose=False):
    """alignment_tools.py:356-419 — translation between two point sets without any image: every pair of target
    points votes, through the pairs of fixed points that are equally far apart (within ``cutoff``), for the
    translations that would map the pair's ends onto the first point of such a fixed pair; the fullest cell of
    the 3-D histogram of votes (cells of ``xyz_res``) gives a rough translation, and the median offset of the
    points that then pair up within ``2 * xyz_res`` is returned (with the paired fixed / target points if
    ``return_pts``).  Host NumPy/SciPy like the reference (used by ``align_beads(use_fft=False)``)."""
    from scipy.spatial.distance import pdist, cdist
    fix = np.array(cents_fix)
    tar = np.array(cents_target)
    if plt_val:
        raise NotImplementedError("plt_val=True (matplotlib figures) is not provided")
    i_fix, j_fix = np.triu_indices(len(fix), 1)          # pairs in the order of pdist / itertools.combinations
    i_tar, j_tar = np.triu_indices(len(tar), 1)
    d_fix, d_tar = pdist(fix), pdist(tar)
    votes = []
    for dt, a, b in zip(d_tar, i_tar, j_tar):
        first = fix[i_fix[np.abs(d_fix - dt) < cutoff]]  # first point of every fixed pair of that length
        votes.append(first - tar[a])
        votes.append(first - tar[b])
    votes = np.concatenate(votes) if votes else np.zeros((0, fix.shape[1]))
    nbins = np.array((np.max(votes, axis=0) - np.min(votes, axis=0)) / float(xyz_res), dtype=int)
    hist, edges = np.histogramdd(votes, bins=nbins)
    best = np.unravel_index(np.argmax(hist), hist.shape)
    rough = np.array([e[k] for e, k in zip(edges, best)])
    nearest = np.argmin(cdist(fix, tar + rough), axis=1)   # for every fixed point its closest shifted target point
    ok = np.sqrt(np.sum((tar[nearest] + rough - fix) ** 2, axis=-1)) < 2 * xyz_res
    pair_fix, pair_tar = fix[ok], tar[nearest[ok]]
    if len(pair_fix) == 0:
        raise ValueError("No matched points exist in cents[inds_closestF]")
    shift = np.median(pair_tar - pair_fix, axis=0)
    if verbose:
        print(f"--- {len(pair_fix)} points are aligned")
    if return_pts:
        return shift, pair_fix, pair_tar
    return shift
