"""Bleedthrough correction profiles (reference: correction_tools/bleedthrough.py), under the reference's names.

``find_bleedthrough_pairs`` keeps the corrected channels of a movie resident, fits the reference channel and makes all
boxes and regressions of a target channel in one ``ia3_crop_pairs_dev`` call; ``check_bleedthrough_info``,
``check_bleedthrough_pairs`` and the two least-squares fits of ``interploate_bleedthrough_correction_from_channel`` are
host code on a few hundred pairs.  The tail of ``Generate_bleedthrough_correction`` (:451-486: the dense slope fields, the
mean over z and one matrix inverse per pixel) is one kernel, ``ia3_bleedthrough_profile_dev`` (csrc/calib.hip), fed with
the polynomial constants of the six directions.  ``bleedthrough_profile_from_pairs`` leaves that profile in HBM for
``correct_fov_image(bleed_profile=...)``."""
import os
import pickle
import time
import numpy as np

from .. import _allowed_colors, _image_size, _correction_folder
from .. import _lib as L
from ..io_tools.load import correct_fov_image, DeviceBuffer
from ..io_tools.crop import _box_sizes
from ..spot_tools.fitting import fit_fov_image
from .chromatic import generate_polynomial_data

# default parameters for bleedthrough profiles (:19-35)
_bleedthrough_channels = ['750', '647', '561']

_bleedthrough_default_correction_args = {
    'correction_folder': _correction_folder,
    'single_im_size': _image_size,
    'all_channels': _allowed_colors,
    'bleed_corr': False,
    'illumination_corr': False,
    'chromatic_corr': False,
    'z_shift_corr': True,
}

_bleedthrough_default_fitting_args = {
    'max_num_seeds': 500,
    'th_seed': 300,
    'use_dynamic_th': True,
}


def check_bleedthrough_info(
        _info,
        _rsq_th=0.81, _intensity_th=150.,
        _check_center_position=True, _center_radius=1.):
    """Function to check one bleedthrough pair (:37-52): r2, fitted height, and the brightest voxel of the reference
    box, which fails only when it lies outside the centre radius on every axis on the same side."""
    if _info['rsquare'] < _rsq_th:
        return False
    elif 'spot' in _info and _info['spot'][0] < _intensity_th:
        return False
    elif _check_center_position:
        _max_inds = np.array(np.unravel_index(np.argmax(_info['ref_im']), np.shape(_info['ref_im'])))
        _im_ct_inds = (np.array(np.shape(_info['ref_im'])) - 1) / 2
        if (_max_inds < _im_ct_inds - _center_radius).all() or (_max_inds > _im_ct_inds + _center_radius).all():
            return False
    return True


def _temp_filename(filename, _channel, _ch):
    _basename = os.path.basename(filename).replace('.dax', f'_ref_{_channel}_to_{_ch}.pkl')
    return os.path.join(os.path.dirname(filename), 'bleedthrough_' + _basename)


def find_bleedthrough_pairs(filename, channel,
                            corr_channels=_bleedthrough_channels,
                            correction_args=_bleedthrough_default_correction_args,
                            fitting_args=_bleedthrough_default_fitting_args,
                            intensity_th=1.,
                            crop_size=9, rsq_th=0.81,
                            check_center_position=True,
                            save_temp=True, save_name=None,
                            overwrite=True, verbose=True,
                            ):
    """Function to generate bleedthrough spot pairs (:56-168): ``{'<ch>_to_<target>': [info, ...]}`` for the spots fitted
    in ``channel`` of the movie, the infos that pass ``check_bleedthrough_info``.  An info holds 'coord' and 'spot'
    (float32 rows of ``fit_fov_image``), 'ref_im' / 'bleed_im' (uint16 boxes of ``crop_size``), 'rsquare', 'slope',
    'intercept' (np.float64) and 'file'; 'rsquare' is a float.

    The corrected channels stay resident from ``correct_fov_image`` through the fit; the boxes and regressions of one
    target channel come from one ``ia3_crop_pairs_dev`` call.  The temp files
    ``bleedthrough_<movie>_ref_<ch>_to_<target>.pkl`` are read (unless ``overwrite``) and written (``save_temp``) as the
    reference does: when only some of them exist the loaded lists are kept and the new pairs are appended to them."""
    _channel = str(channel)
    if _channel not in corr_channels:
        raise ValueError(f"{_channel} should be within {corr_channels}")

    _info_dict = {}
    _load_flags = []
    for _ch in corr_channels:
        if _ch != _channel:
            _fl = _temp_filename(filename, _channel, _ch)
            if os.path.isfile(_fl) and not overwrite:
                with open(_fl, 'rb') as _f:
                    _infos = pickle.load(_f)
                _info_dict[f"{_channel}_to_{_ch}"] = [
                    _info for _info in _infos
                    if check_bleedthrough_info(_info, _rsq_th=rsq_th, _intensity_th=intensity_th,
                                               _check_center_position=check_center_position)]
                _load_flags.append(1)
            else:
                _info_dict[f"{_channel}_to_{_ch}"] = []
                _load_flags.append(0)

    if np.mean(_load_flags) == 1:
        if verbose:
            print(f"-- directly load from saved tempfile in folder: {os.path.dirname(filename)}")
        return _info_dict

    _held = []
    try:
        # the corrected channels of the movie, resident
        _ims = correct_fov_image(filename, corr_channels,
                                 calculate_drift=False, warp_image=False,
                                 **correction_args,
                                 return_drift=False, verbose=verbose, return_device=True)[0]
        _held += list(_ims)
        # spots of the labelled channel
        _ref_im = _ims[list(corr_channels).index(_channel)]
        _tar_channels = [_ch for _ch, _im in zip(corr_channels, _ims) if _ch != _channel]
        _tar_ims = [_im for _ch, _im in zip(corr_channels, _ims) if _ch != _channel]
        _ref_spots = fit_fov_image(_ref_im, _channel, **fitting_args, verbose=verbose)
        # per target channel: x = the labelled channel's box, y = the target's box at the same centre (:122-128)
        for _ch, _im in zip(_tar_channels, _tar_ims):
            _key = f"{_channel}_to_{_ch}"
            if verbose:
                print(f"--- finding matched bleedthrough pairs for {_key}")
            if len(_ref_spots) == 0:
                continue
            _cts = _ref_spots[:, 1:4]
            _rims, _cims, (_slopes, _intercepts, _rsqs) = L.crop_pairs(
                _ref_im, _cts, _box_sizes(crop_size), _im, _cts, regress=True)
            for _k, _spot in enumerate(_ref_spots):
                _info_dict[_key].append({
                    'coord': _spot[1:4],
                    'spot': _spot,
                    'ref_im': _rims[_k].copy(),
                    'bleed_im': _cims[_k].copy(),
                    'rsquare': float(_rsqs[_k]),
                    'slope': np.float64(_slopes[_k]),
                    'intercept': np.float64(_intercepts[_k]),
                    'file': filename,
                })
    finally:
        for _im in _held:
            if isinstance(_im, L.DeviceStack):
                _im.free()

    if save_temp:
        for _ch in corr_channels:
            if _ch != _channel:
                _key = f"{_channel}_to_{_ch}"
                _fl = _temp_filename(filename, _channel, _ch)
                if verbose:
                    print(f"--- saving {len(_info_dict[_key])} points to file:{_fl}")
                with open(_fl, 'wb') as _f:
                    pickle.dump(_info_dict[_key], _f)
            else:
                if verbose:
                    print(f"-- channel {_ch} doesn't match {_channel}, skip saving.")

    # what is handed back is filtered; the temp files hold every pair
    _kept_info_dict = {_key: [] for _key in _info_dict}
    for _key, _infos in _info_dict.items():
        _kept_info_dict[_key] = [
            _info for _info in _infos
            if check_bleedthrough_info(_info, _rsq_th=rsq_th, _intensity_th=intensity_th,
                                       _check_center_position=check_center_position)]
    return _kept_info_dict


def _delaunay_neighbors(simplices, n):
    """Per point 0..n-1 the sorted ids of every point it shares a simplex with, itself included (empty for a point
    in no simplex): what ``np.unique`` of the simplices holding the point gives."""
    _s = np.asarray(simplices, dtype=int)
    _w = _s.shape[1]
    _a = np.repeat(_s, _w, axis=1).ravel()
    _b = np.tile(_s, (1, _w)).ravel()
    _pairs = np.unique(_a * np.int64(n) + _b)
    _a, _b = _pairs // n, _pairs % n
    _starts = np.searchsorted(_a, np.arange(n + 1))
    return [_b[_starts[_i]:_starts[_i + 1]] for _i in range(n)]


def check_bleedthrough_pairs(info_list, outlier_sigma=2, keep_per_th=0.95, max_iter=20,
                             verbose=True, ):
    """Function to check bleedthrough pairs (:171-231): drops, round after round, the pairs whose slope or intercept is
    further than ``outlier_sigma`` standard deviations of its Delaunay neighbours' from their distance-weighted mean,
    until a round keeps ``keep_per_th`` of them.

    The neighbour sets come from one pass over the simplices; the arithmetic per point is the reference's, including
    that a neighbour id counted among the pairs still kept is looked up in the arrays of all pairs (:203-205)."""
    from scipy.spatial import Delaunay
    if verbose:
        print(f"- check {len(info_list)} bleedthrough pairs.")
    _coords = np.array([_info['coord'] for _info in info_list])
    _slopes = np.array([_info['slope'] for _info in info_list])
    _intercepts = np.array([_info['intercept'] for _info in info_list])

    if verbose:
        print(f"- start iteration with outlier_sigma={outlier_sigma:.2f}, keep_percentage={keep_per_th:.2f}")
    _n_iter = 0
    _kept_flags = np.ones(len(_coords), dtype=bool)
    _flags = []
    while (len(_flags) == 0 or np.mean(_flags) < keep_per_th):
        _n_iter += 1
        _start_time = time.time()
        _flags = []
        _tri = Delaunay(_coords[_kept_flags])
        _neighbors = _delaunay_neighbors(_tri.simplices, int(np.sum(_kept_flags)))
        for _i, (_coord, _slope, _intercept) in enumerate(zip(_coords[_kept_flags],
                                                              _slopes[_kept_flags],
                                                              _intercepts[_kept_flags])):
            _nb_ids = _neighbors[_i]
            _nb_ids = _nb_ids[(_nb_ids != _i) & (_nb_ids != -1)]
            _nb_coords = _coords[_nb_ids]
            _nb_slopes = _slopes[_nb_ids]
            _nb_intercepts = _intercepts[_nb_ids]
            with np.errstate(divide='ignore', invalid='ignore'):
                _nb_weights = 1 / np.linalg.norm(_nb_coords - _coord, axis=1)
                _nb_weights = _nb_weights / np.sum(_nb_weights)
                # distance-weighted mean of the neighbours against the pair's own value, slope then intercept
                _exp_slope = np.dot(_nb_slopes.T, _nb_weights)
                _keep_slope = (np.abs(_exp_slope - _slope) <= outlier_sigma * _std(_nb_slopes))
                _exp_intercept = np.dot(_nb_intercepts.T, _nb_weights)
                _keep_intercept = (np.abs(_exp_intercept - _intercept) <= outlier_sigma * _std(_nb_intercepts))
            _flags.append((_keep_slope and _keep_intercept))

        # the flags of this round belong to the pairs that entered it
        _updating_inds = np.where(_kept_flags)[0]
        _kept_flags[_updating_inds] = np.array(_flags, dtype=bool)
        if verbose:
            print(f"-- iter: {_n_iter}, kept in this round: {np.mean(_flags):.3f}, total: {np.mean(_kept_flags):.3f} in {time.time()-_start_time:.3f}s")
        if _n_iter > max_iter:
            if verbose:
                print(f"-- stopped after {_n_iter} rounds (max_iter={max_iter}).")
            break
    kept_info_list = [_info for _info, _flag in zip(info_list, _kept_flags) if _flag]
    if verbose:
        print(f"- {len(kept_info_list)} pairs passed.")
    return kept_info_list


def _std(_v):
    """``np.std``; of no values NaN, without NumPy's warnings."""
    return np.std(_v) if len(_v) > 0 else np.nan


def _bleedthrough_constants(info_dicts, ref_channel, target_channel,
                            check_info=True, check_params={},
                            max_num_spots=1000, min_num_spots=100,
                            fitting_order=2, verbose=True):
    """The first half of ``interploate_bleedthrough_correction_from_channel`` (:248-309): selection of the pairs of
    ``<ref>_to_<target>``, the check, and the two least-squares fits of slope and intercept on the columns of
    ``generate_polynomial_data`` of the uncentred coordinates (:298).  Returns ``(C_slope, C_intercept, rsq_slope,
    rsq_intercept)``, or None when fewer than ``min_num_spots`` pairs are there (the zero profile)."""
    import scipy.linalg
    _key = f"{ref_channel}_to_{target_channel}"
    _info_list = []
    for _dict in info_dicts:
        if _key in _dict:
            _info_list += list(_dict[_key])
    if len(_info_list) < min_num_spots:
        if verbose:
            print(f"-- {_key}: {len(_info_list)} pairs, fewer than min_num_spots={min_num_spots}: zero profile")
        return None
    # at most max_num_spots pairs, those of highest r2 (ties at the threshold all stay, :262-265)
    if len(_info_list) > max_num_spots:
        if verbose:
            print(f"-- only keep the top {max_num_spots} spots from {len(_info_list)} for bleedthrough interpolation.")
    if len(_info_list) > int(max_num_spots):
        _rsquares = np.array([_info['rsquare'] for _info in _info_list])
        _rsq_th = np.sort(_rsquares)[-int(max_num_spots)]
        _info_list = [_info for _info in _info_list if _info['rsquare'] >= _rsq_th]
    if check_info:
        _info_list = check_bleedthrough_pairs(_info_list, **check_params)
    _coords = [_info['coord'] for _info in _info_list]
    _slopes = [_info['slope'] for _info in _info_list]
    _intercepts = [_info['intercept'] for _info in _info_list]
    if len(_coords) < min_num_spots:
        if verbose:
            print(f"-- {_key}: {len(_coords)} pairs left after the check, fewer than min_num_spots={min_num_spots}: zero profile")
        return None
    if verbose:
        print(f"-- {len(_coords)} spots are used to generate profiles from {ref_channel} to {target_channel}")
    _coords = np.array(_coords)
    _slopes = np.array(_slopes)
    _intercepts = np.array(_intercepts)
    # generate_polynomial_data of the coordinates as fitted, not moved to the reference centre (:298)
    _X = generate_polynomial_data(_coords, fitting_order)
    _C_slope, _r, _r2, _r3 = scipy.linalg.lstsq(_X, _slopes)
    _rsq_slope = 1 - np.sum((_X.dot(_C_slope) - _slopes)**2) \
        / np.sum((_slopes - np.mean(_slopes))**2)
    _C_intercept, _r, _r2, _r3 = scipy.linalg.lstsq(_X, _intercepts)
    _rsq_intercept = 1 - np.sum((_X.dot(_C_intercept) - _intercepts)**2) \
        / np.sum((_intercepts - np.mean(_intercepts))**2)
    if verbose:
        print(_C_slope, _rsq_slope)
        print(_C_intercept, _rsq_intercept)
    return _C_slope, _C_intercept, _rsq_slope, _rsq_intercept


def _profile_center(single_im_size, ref_center):
    """:291-294 for three coordinates."""
    if ref_center is None:
        return np.array(single_im_size)[:3] / 2
    return np.array(ref_center)[:3]


def _slope_intercept_fields(fit, fitting_order, ref_center, shape):
    """The dense (Z, X, Y) slope and intercept fields of one direction's constants (:312-318), downloaded: slope,
    intercept and an order-0 zero as the three "axes" of one ``ia3_poly_field_dev`` call."""
    _buf = DeviceBuffer.adopt(L.poly_field([fit[0], fit[1], np.zeros(1)], [int(fitting_order), int(fitting_order), 0],
                                           ref_center, shape, np.float64), (3,) + tuple(shape), np.float64)
    try:
        return _buf.download()
    finally:
        _buf.free()


def interploate_bleedthrough_correction_from_channel(
        info_dicts, ref_channel, target_channel,
        check_info=True, check_params={},
        max_num_spots=1000, min_num_spots=100,
        single_im_size=_image_size, ref_center=None,
        fitting_order=2, allow_intercept=True,
        save_temp=True, save_folder=None,
        make_plots=True, save_plots=True,
        overwrite=False, verbose=True,
        ):
    """Function to interpolate and generate the bleedthrough correction profiles between two channels (:235-349):
    ``(slope profile, intercept profile)``, two float64 (Z, X, Y) arrays; zeros when fewer than ``min_num_spots`` pairs
    are there.

    The profiles are the fitted polynomials at pixel coordinates minus ``ref_center`` (:314-316), made in one
    ``ia3_poly_field_dev`` call and downloaded.  Figures go through matplotlib's Agg backend, are saved when
    ``save_plots`` is set and ``save_folder`` is a folder, and are never shown."""
    _shape = tuple(int(_d) for _d in single_im_size)
    _fit = _bleedthrough_constants(info_dicts, ref_channel, target_channel, check_info, check_params,
                                   max_num_spots, min_num_spots, fitting_order, verbose)
    if _fit is None:
        return np.zeros(single_im_size), np.zeros(single_im_size)
    _C_slope, _C_intercept, _rsq_slope, _rsq_intercept = _fit
    _ref_center = _profile_center(single_im_size, ref_center)
    _fields = _slope_intercept_fields(_fit, fitting_order, _ref_center, _shape)
    _p_slope, _p_intercept = _fields[0].copy(), _fields[1].copy()
    if save_temp:
        if save_folder is not None and os.path.isdir(save_folder):
            if verbose:
                print(f"-- saving bleedthrough temp profile from channel: {ref_channel} to channel: {target_channel}.")
        else:
            print(f"-- save_folder is not given or not valid, skip.")
    if make_plots:
        _plot_bleedthrough(_p_slope.mean(0), _p_intercept.mean(0), _rsq_slope, _rsq_intercept, ref_channel, target_channel,
                           save_folder if (save_plots and save_folder is not None and os.path.isdir(save_folder)) else None,
                           verbose)
    return _p_slope, _p_intercept


def _plot_bleedthrough(slope_map, intercept_map, rsq_slope, rsq_intercept, ref_channel, target_channel, folder, verbose):
    """The figures of :330-347 from the (X, Y) z-means of the two profiles, through the Agg backend:
    ``bleedthrough_profile_<ref>_to_<target>_<slope|intercept>.png`` in ``folder`` when one is given."""
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except Exception as _e:
        if verbose:
            print(f"-- make_plots: matplotlib is not available ({_e}), no figure is drawn")
        return
    for _pf, _rsq, _name in ((slope_map, rsq_slope, 'slope'), (intercept_map, rsq_intercept, 'intercept')):
        _fig = plt.figure(dpi=150, figsize=(4, 3))
        plt.imshow(_pf)
        plt.colorbar()
        plt.title(f"{ref_channel} to {target_channel}, {_name}, rsq={_rsq:.3f}")
        if folder is not None:
            _fig.savefig(os.path.join(folder, f'bleedthrough_profile_{ref_channel}_to_{target_channel}_{_name}.png'),
                         transparent=True)
        plt.close(_fig)


def _profile_arguments(info_dicts, corr_channels, fitting_order, interpolate_args, verbose=True):
    """(consts (C, C, n_cols), present (C, C), per-direction fits) of every direction ref -> target, in the order the
    reference visits them (:458-470); ``consts[tar, ref]`` is the slope polynomial."""
    _args = dict(interpolate_args)
    _unknown = set(_args) - {'check_info', 'check_params', 'max_num_spots', 'min_num_spots', 'ref_center',
                             'allow_intercept', 'save_temp', 'make_plots', 'save_plots', 'overwrite'}
    if _unknown:
        raise TypeError(f"interploate_bleedthrough_correction_from_channel() got unexpected arguments {sorted(_unknown)}")
    _nc = len(corr_channels)
    _order = int(fitting_order)
    if _order < 0:
        raise ValueError(f"fitting order {_order} should not be negative")
    if _order > 3:
        raise NotImplementedError(f"fitting order {_order}: the device profile is built for orders 0 to 3")
    _consts = np.zeros((_nc, _nc, L.poly_columns(_order)), dtype=np.float64)
    _present = np.zeros((_nc, _nc), dtype=np.uint8)
    _fits = {}
    for _ref_i, _ref_ch in enumerate(corr_channels):
        for _tar_i, _tar_ch in enumerate(corr_channels):
            if _ref_ch == _tar_ch:
                continue
            _fit = _bleedthrough_constants(info_dicts, _ref_ch, _tar_ch,
                                           _args.get('check_info', True), _args.get('check_params', {}),
                                           _args.get('max_num_spots', 1000), _args.get('min_num_spots', 100),
                                           _order, verbose)
            _fits[(_ref_ch, _tar_ch)] = _fit
            if _fit is not None:
                _consts[_tar_i, _ref_i] = _fit[0]
                _present[_tar_i, _ref_i] = 1
    return _consts, _present, _fits


def bleedthrough_profile_from_pairs(info_dicts, corr_channels=_bleedthrough_channels, single_im_size=_image_size,
                                    fitting_order=2, generate_2d=True, interpolate_args={}, ref_center=None,
                                    invert=True, verbose=True, dtype=np.float32):
    """The bleedthrough profile of the pairs ``find_bleedthrough_pairs`` returned (a list of its dicts), made in HBM
    and left there: a ``DeviceBuffer`` of shape (C, C, X, Y) (``generate_2d``) or (C, C, Z, X, Y), ready for
    ``correct_fov_image(bleed_profile=...)`` without the ``.npy`` in between.  float64 holds what
    ``Generate_bleedthrough_correction`` saves; float32 the same values rounded once (what the corrections read).
    ``invert=False`` gives the mixing matrices themselves (:456-475)."""
    _shape = tuple(int(_d) for _d in single_im_size)
    if len(_shape) != 3:
        raise ValueError("single_im_size should be (Z, X, Y)")
    _args = dict(interpolate_args)
    if ref_center is not None:
        _args['ref_center'] = ref_center
    _consts, _present, _ = _profile_arguments(info_dicts, corr_channels, fitting_order, _args, verbose)
    _center = _profile_center(single_im_size, _args.get('ref_center', None))
    _p = L.bleedthrough_profile(_consts, _present, fitting_order, _center, _shape, mean_z=bool(generate_2d),
                                invert=bool(invert), dtype=dtype)
    _nc = len(corr_channels)
    return DeviceBuffer.adopt(_p, (_nc, _nc) + (_shape[1:] if generate_2d else _shape), dtype)


def Generate_bleedthrough_correction(bleed_folders,
                                     corr_channels=_bleedthrough_channels,
                                     parallel=True, num_threads=12,
                                     start_fov=1, num_images=40,
                                     correction_args={'single_im_size': _image_size,
                                                      'illumination_corr': False,
                                                      'chromatic_corr': False},
                                     fitting_args={}, intensity_th=150.,
                                     crop_size=9, rsq_th=0.81, check_center=True,
                                     fitting_order=2, generate_2d=True,
                                     interpolate_args={},
                                     make_plots=True, save_plots=True,
                                     save_folder=None,
                                     save_name='bleedthrough_correction',
                                     overwrite_temp=False, overwrite_profile=False,
                                     verbose=True,
                                     ):
    """Function to generate bleedthrough profiles (:353-496) from one folder of movies per channel of ``corr_channels``
    (folder k holds the movies in which only channel k is labelled): the float64 (C, C, X, Y) (``generate_2d``) or
    (C, C, Z, X, Y) array whose [:, :, x, y] is the inverse of the matrix of bleedthrough slopes at that pixel, saved
    reshaped to (C*C, ...) as ``<save_name>_<channels>_<X>_<Y>.npy`` (``_<Z>_<X>_<Y>``) in ``save_folder``; an existing
    file is loaded and returned as it is (C*C first) unless ``overwrite_profile``.

    ``parallel`` / ``num_threads`` are accepted; the movies go through the device one after the other in this process.
    The six polynomial fits feed one ``ia3_bleedthrough_profile_dev`` call, downloaded once.  ``make_plots`` (and
    ``interpolate_args['make_plots']``, the only switch the reference's call honours) draws the slope and intercept maps
    of every direction (z-means from two more calls of the same kernel, without inversion) through the Agg backend; they
    are saved when ``save_plots`` is set and never shown."""
    # defaults, overridden by what the caller gives
    _correction_args = {_k: _v for _k, _v in _bleedthrough_default_correction_args.items()}
    _correction_args.update(correction_args)
    _fitting_args = {_k: _v for _k, _v in _bleedthrough_default_fitting_args.items()}
    _fitting_args.update(fitting_args)
    # <save_name>_<channels>_<dims>.npy, the dims being (X, Y) or (Z, X, Y)
    if save_folder is None:
        save_folder = bleed_folders[0]
    filename_base = save_name
    for _ch in corr_channels:
        filename_base += f"_{_ch}"
    if generate_2d:
        for _d in _correction_args['single_im_size'][-2:]:
            filename_base += f'_{int(_d)}'
    else:
        for _d in _correction_args['single_im_size']:
            filename_base += f'_{int(_d)}'
    saved_profile_filename = os.path.join(save_folder, filename_base + '.npy')
    if os.path.isfile(saved_profile_filename) and not overwrite_profile:
        if verbose:
            print(f"+ bleedthrough correction profiles already exists. direct load the profile")
        _bleed_profiles = np.load(saved_profile_filename, allow_pickle=True)
    else:
        if verbose:
            print(f"+ generating bleedthrough profiles.")
        # the movies of the first folder in the order of their numbers, from start_fov on
        fov_names = [_fl for _fl in os.listdir(bleed_folders[0]) if _fl.split('.')[-1] == 'dax']
        sel_fov_names = [_fl for _fl in sorted(fov_names, key=lambda v: int(v.split('.dax')[0].split('_')[-1]))]
        sel_fov_names = sel_fov_names[int(start_fov):int(start_fov) + int(num_images)]
        # one find_bleedthrough_pairs call per movie and labelled channel, in the reference's argument order
        _bleed_args = []
        for _fov in sel_fov_names:
            for _folder, _ch in zip(bleed_folders, corr_channels):
                _bleed_args.append((os.path.join(_folder, _fov), _ch, corr_channels, _correction_args, _fitting_args,
                                    intensity_th, crop_size, rsq_th, check_center, True, None, overwrite_temp, verbose))
        if verbose:
            print(f"++ generating bleedthrough info for {len(sel_fov_names)} images in", end=' ')
            _multi_start = time.time()
        _info_dicts = [find_bleedthrough_pairs(*_arg) for _arg in _bleed_args]
        if verbose:
            print(f"{time.time()-_multi_start:.3f}s.")
        # the fits on the host; the fields, the mean over z and the inverses in one kernel
        _size = _correction_args['single_im_size']
        _shape = tuple(int(_d) for _d in _size)
        _consts, _present, _fits = _profile_arguments(_info_dicts, corr_channels, fitting_order, interpolate_args, True)
        _center = _profile_center(_size, interpolate_args.get('ref_center', None))
        if verbose:
            print(f"-- generating inverse matrix.")
        _nc = len(corr_channels)
        _buf = DeviceBuffer.adopt(L.bleedthrough_profile(_consts, _present, fitting_order, _center, _shape,
                                                         mean_z=bool(generate_2d), invert=True, dtype=np.float64),
                                  (_nc, _nc) + (_shape[1:] if generate_2d else _shape), np.float64)
        try:
            _bleed_profiles = _buf.download()
        finally:
            _buf.free()
        if make_plots and interpolate_args.get('make_plots', True):
            # the z-means the figures show are two (C, C, X, Y) forward profiles: the slopes', and the same kernel on the
            # intercepts' constants; no dense field is built or downloaded for them
            _folder = save_folder if (save_plots and interpolate_args.get('save_plots', True)
                                      and os.path.isdir(save_folder)) else None
            _chs = list(corr_channels)
            _icpt_consts = np.zeros_like(_consts)
            for (_ref_ch, _tar_ch), _fit in _fits.items():
                if _fit is not None:
                    _icpt_consts[_chs.index(_tar_ch), _chs.index(_ref_ch)] = _fit[1]
            _maps = []
            for _c in (_consts, _icpt_consts):
                _mbuf = DeviceBuffer.adopt(L.bleedthrough_profile(_c, _present, fitting_order, _center, _shape, mean_z=True,
                                                                  invert=False, dtype=np.float64),
                                           (_nc, _nc) + _shape[1:], np.float64)
                try:
                    _maps.append(_mbuf.download())
                finally:
                    _mbuf.free()
            for (_ref_ch, _tar_ch), _fit in _fits.items():
                if _fit is not None:
                    _t, _r = _chs.index(_tar_ch), _chs.index(_ref_ch)
                    _plot_bleedthrough(_maps[0][_t, _r], _maps[1][_t, _r], _fit[2], _fit[3], _ref_ch, _tar_ch, _folder, verbose)
        # saved whatever verbose says, C * C first (:492)
        if verbose:
            print(f"-- saving to file:{saved_profile_filename}")
        np.save(saved_profile_filename,
                _bleed_profiles.reshape(np.concatenate([[len(corr_channels)**2], np.shape(_bleed_profiles)[2:]])))
    return _bleed_profiles
