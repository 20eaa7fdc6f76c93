"""Drop-in for the reference's ``correction_tools/illumination.py`` — same names, signatures and defaults.

The per-image work of ``_image_to_profile`` (two stack percentiles, clip, sum over z, float64 Gaussian) runs on the
device on the stacks ``correct_fov_image(..., return_device=True)`` leaves resident (``ia3_illumination_image_profile_dev``,
csrc/stats.hip); results equal the reference's bit for bit.  All ``file:line`` citations are relative to the reference
tree.
"""
import os
import time
import numpy as np

from .. import _allowed_colors, _image_size, _correction_folder
from .. import _lib as L


def _gaussian_filter_f64(im, sigma):
    """``scipy.ndimage.gaussian_filter(im, sigma)`` of a float64 2-D image on the device (ia3_gaussian_filter2d_f64,
    taps from NumPy as SciPy makes them)."""
    return L.gaussian_filter2d_f64(im, sigma)


def _stack_to_profile(stack, remove_cap=True, cap_th_per=[5, 90], gaussian_filter_size=40):
    """correction_tools/illumination.py:181-190 for one channel image: a resident ``DeviceStack`` or a (Z,X,Y) uint16 /
    float32 ndarray (uploaded for the call).  Returns the float64 (X, Y) profile."""
    _resident = isinstance(stack, L.DeviceStack)
    _st = stack if _resident else L.DeviceStack.upload(stack)
    try:
        _out = np.empty(tuple(_st.shape[1:]), dtype=np.float64)
        _wp, _r, _keep = L.taps_argument(gaussian_filter_size)
        L.check(L.lib().ia3_illumination_image_profile_dev(
            _st._h, 1 if remove_cap else 0, float(min(cap_th_per)), float(max(cap_th_per)),
            float(gaussian_filter_size), _wp, _r, L.dptr(_out)))
    finally:
        if not _resident:
            _st.free()
    return _out


def Generate_illumination_correction(data_folder,
                                     sel_channels=None,
                                     num_threads=12, parallel=True,
                                     num_images=48,
                                     single_im_size=_image_size, all_channels=_allowed_colors,
                                     num_buffer_frames=10, num_empty_frames=0,
                                     correction_folder=_correction_folder,
                                     hot_pixel_corr=True, hot_pixel_th=4, z_shift_corr=True,
                                     remove_cap=True, cap_th_per=[5, 90],
                                     gaussian_filter_size=60,
                                     save=True, overwrite=False, save_folder=None,
                                     save_prefix='illumination_correction_',
                                     make_plot=True, verbose=True):
    """correction_tools/illumination.py:16-142 — illumination profiles of the selected channels from the first
    ``num_images`` movies of ``data_folder``: list of float64 (X, Y) arrays in the order of ``sel_channels``.

    ``parallel`` / ``num_threads`` are accepted; the images go through the device one after the other in this process
    (no ``mp.Pool``: the GPU is never opened before a fork).  Figures are written with matplotlib's Agg backend when
    ``save`` is set and matplotlib is installed, and never shown."""
    _total_start = time.time()
    if sel_channels is None:
        sel_channels = all_channels
    if save_folder is None:
        save_folder = os.path.join(data_folder, 'Corrections')
    if not os.path.isdir(save_folder):
        os.makedirs(save_folder)
    _save_filenames = [os.path.join(save_folder, f"{save_prefix}{_ch}_{single_im_size[-2]}x{single_im_size[-1]}.npy")
                       for _ch in sel_channels]
    # channels whose file exists are loaded (:50-57)
    _exists = [os.path.isfile(_fl) and not overwrite for _fl in _save_filenames]
    _loaded_pfs = [np.load(_fl) for _fl, _e in zip(_save_filenames, _exists) if _e]
    _loaded_channels = [_ch for _ch, _e in zip(sel_channels, _exists) if _e]
    if verbose:
        print(f"-- directly load:{_loaded_channels} illumination profiles for files")
    _sel_channels = [_ch for _ch, _e in zip(sel_channels, _exists) if not _e]
    _sel_filenames = [_fl for _fl, _e in zip(_save_filenames, _exists) if not _e]
    _sel_pfs = []
    if len(_sel_channels) > 0:
        if verbose:
            print(f"-- start calculating {_sel_channels} illumination profiles")
        _fovs = [_fl for _fl in os.listdir(data_folder) if _fl.split('.')[-1] == 'dax']           # :64-70
        _fovs = sorted(_fovs, key=lambda v: int(v.split('.dax')[0].split('_')[-1]))
        _num_load = min(num_images, len(_fovs))
        if verbose:
            print(f"-- {_num_load} among {len(_fovs)} dax files will be loaded in data_folder: {data_folder}")
        _input_fls = [os.path.join(data_folder, _fl) for _fl in _fovs[:_num_load]]
        if verbose:
            _multi_time = time.time()
            print(f"++ start illumination profile calculateion for {len(_input_fls)} images")
        _pfs_per_fov = [_image_to_profile(_fl, _sel_channels, remove_cap, cap_th_per, gaussian_filter_size,
                                          single_im_size, all_channels, num_buffer_frames, num_empty_frames,
                                          hot_pixel_corr, hot_pixel_th, z_shift_corr, verbose)
                        for _fl in _input_fls]
        if verbose:
            print(f"finish in {time.time()-_multi_time:.2f}s.")
        for _i, _ch in enumerate(_sel_channels):                                                  # :104-109
            _pf = np.mean([_r[_i] for _r in _pfs_per_fov], axis=0)
            _pf = _gaussian_filter_f64(_pf, gaussian_filter_size)
            _sel_pfs.append(_pf / np.max(_pf))
        if save:
            if verbose:
                print("-- saving updated profiles")
            for _ch, _pf, _fl in zip(_sel_channels, _sel_pfs, _sel_filenames):
                if verbose:
                    print(f"--- saving {_ch} profile into file: {_fl}")
                np.save(_fl.split('.npy')[0], _pf)
    _illumination_pfs = []                                                                        # :121-129
    for _ch in sel_channels:
        if _ch in _sel_channels:
            _illumination_pfs.append(_sel_pfs[_sel_channels.index(_ch)])
        elif _ch in _loaded_channels:
            _illumination_pfs.append(_loaded_pfs[_loaded_channels.index(_ch)])
        else:
            raise IndexError(f"channel: {_ch} doesn't exist in either _sel_channels or _loaded_channels!")
    if make_plot:
        _plot_profiles(sel_channels, _illumination_pfs, _save_filenames, save, verbose)
    if verbose:
        print(f"-- finish generating illumination profiles, time:{time.time()-_total_start:.2f}s")
    return _illumination_pfs


def _plot_profiles(channels, profiles, filenames, save, verbose):
    """The figures of correction_tools/illumination.py:131-139, written to ``<profile>.png`` and never shown."""
    if not save:
        if verbose:
            print("-- make_plot: nothing is saved, so no figure is drawn")
        return
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except Exception as _e:
        if verbose:
            print(f"-- make_plot: matplotlib is not available ({_e}), no figure is drawn")
        return
    for _ch, _pf, _fl in zip(channels, profiles, filenames):
        _fig = plt.figure(dpi=150, figsize=(4, 3))
        plt.imshow(_pf)
        plt.colorbar()
        plt.title(f"illumination, channel:{_ch}")
        _fig.savefig(_fl.replace('.npy', '.png'), transparent=True)
        plt.close(_fig)


def _image_to_profile(filename, sel_channels,
                      remove_cap=True, cap_th_per=[5, 90],
                      gaussian_filter_size=40,
                      single_im_size=_image_size,
                      all_channels=_allowed_colors,
                      num_buffer_frames=10, num_empty_frames=0,
                      hot_pixel_corr=True, hot_pixel_th=4,
                      z_shift_corr=False,
                      verbose=True,
                      ):
    """correction_tools/illumination.py:146-194 — one movie into one profile per selected channel (list of float64
    (X, Y) arrays).  The channel stacks stay resident between the pre-corrections and the reduction."""
    from ..io_tools.load import correct_fov_image
    if verbose:
        print(f"-- load image: {os.path.join(os.path.basename(filename))} for illumination", end=' ')
        _start_time = time.time()
    _ims, _ = correct_fov_image(filename, sel_channels,
                                single_im_size=single_im_size,
                                all_channels=all_channels,
                                num_buffer_frames=num_buffer_frames,
                                num_empty_frames=num_empty_frames,
                                calculate_drift=False,
                                corr_channels=sel_channels,
                                warp_image=False,
                                hot_pixel_corr=hot_pixel_corr,
                                hot_pixel_th=hot_pixel_th,
                                z_shift_corr=z_shift_corr,
                                illumination_corr=False, chromatic_corr=False,
                                bleed_corr=False,
                                return_drift=False, verbose=verbose, return_device=True)
    if verbose:
        _load_time = time.time()
        print(f"in {_load_time-_start_time:.2f}s,", end=' ')
    _pfs = []
    try:
        for _im, _ch in zip(_ims, sel_channels):
            _pfs.append(_stack_to_profile(_im, remove_cap, cap_th_per, gaussian_filter_size))
    finally:
        for _im in _ims:
            _im.free()
    if verbose:
        print(f"into profile in {time.time()-_load_time:.2f}s.")
    return _pfs


def illumination_correction(im, corr_profile):
    """correction_tools/illumination.py:196-212 — apply a 2-D (x, y) profile to a 2-D or 3-D integer image: the float32
    quotient clipped to the range of the image's dtype.  Host NumPy, as in the reference (the corrected chain of
    ``correct_fov_image`` runs ``ia3_illumination_correct_dev``)."""
    if len(np.shape(corr_profile)) != 2:
        raise IndexError("corr_profile for illumination should be 2d")
    _ndim = len(np.shape(im))
    if _ndim not in (2, 3):
        raise IndexError("input image should be 2d or 3d.")
    _info = np.iinfo(im.dtype)
    _prof = corr_profile[np.newaxis, :] if _ndim == 3 else corr_profile
    return np.clip(im.astype(np.float32) / _prof, a_min=_info.min, a_max=_info.max).astype(im.dtype)
