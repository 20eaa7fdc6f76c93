"""Chromatic-aberration profiles (reference: correction_tools/chromatic.py), under the reference's names.

``generate_chromatic_function`` / ``generate_polynomial_data`` (:41-143): coordinate-space chromatic/drift translation of
spot tables, the alternative to warping the image that ``correct_fov_image(warp_image=False)`` hands back.  Host
arithmetic on (N,3) / (N,11) spot tables — a few thousand rows.

``Generate_chromatic_abbrevation`` / ``find_chromatic_spot_pairs`` (:119-412): the generator of those profiles.  The boxes
around the matched spots and their regressions (``ia3_crop_pairs_dev``) and the dense field (``ia3_poly_field_dev``) are
made on the device, csrc/calib.hip; the two small least-squares fits stay on the host.
``chromatic_profile_from_constants`` builds the dense field of a ``_const.pkl`` in HBM for a production run."""
import itertools
import os
import pickle
import time
import numpy as np

from .. import _allowed_colors, _image_size, _correction_folder
from .. import _lib as L
from . import _drift_channel
from ..io_tools.load import correct_fov_image, DeviceBuffer
from ..io_tools.crop import _box_sizes
from ..spot_tools.fitting import fit_fov_image
from ..spot_tools.matching import find_paired_centers

# required chromatic parameters (:20-38)
_chromatic_ref_channel = '647'

_chromatic_default_correction_args = {
    'correction_folder': _correction_folder,
    'single_im_size': _image_size,
    'all_channels': _allowed_colors,
    'bleed_corr': False,
    'chromatic_corr': False,
}
_chromatic_default_drift_args = {
    'drift_channel': _drift_channel,
    'use_autocorr': True,
}
_chromatic_default_fitting_args = {
    'th_seed': 400,
    'max_num_seeds': 300,
    'use_dynamic_th': True,
}


def generate_polynomial_data(coords, max_order):
    """Columns = all monomials of the coordinate columns up to ``max_order`` (orders ascending, within an order
    ``itertools.combinations_with_replacement`` order), n_points x n_columns (chromatic.py:123-143)."""
    coords = np.asarray(coords)
    cols = coords.transpose()
    feats = []
    for order in range(int(max_order) + 1):
        for combo in itertools.combinations_with_replacement(range(len(cols)), order):
            x = np.ones(coords.shape[0])
            for k in combo:
                x *= cols[k]
            feats.append(x)
    return np.array(feats).transpose()


def generate_chromatic_function(chromatic_const_file, drift=None):
    """chromatic.py:41-115 — returns ``f(coords)`` with ``coords`` (N,ndim) or an (N,11) spot table:
    ``coords - polynomial_shift(coords - ref_center) + drift``."""
    if isinstance(chromatic_const_file, dict):
        info = dict(chromatic_const_file)
    elif isinstance(chromatic_const_file, str):
        with open(chromatic_const_file, 'rb') as f:
            info = pickle.load(f)
    elif chromatic_const_file is None:
        if drift is None:
            return lambda _coords, _drift=None: _coords
        info = {'constants': [np.array([0]) for _ in drift],
                'fitting_orders': np.zeros(len(drift), dtype=int),
                'ref_center': np.zeros(len(drift))}
    else:
        raise TypeError("Wrong input chromatic_const_file")
    consts, orders, ref_center = info['constants'], info['fitting_orders'], info['ref_center']
    nd = len(ref_center)
    shift0 = np.zeros(nd) if drift is None else drift[:nd]

    def _shift_function(_coords, _drift=shift0, _consts=consts, _fitting_orders=orders, _ref_center=ref_center):
        if len(_coords) == 0:
            return _coords
        table = np.array(_coords)
        width = table.shape[1]
        if width == nd:
            pts = table.copy()
        elif width == 11:
            pts = table[:, 1:1 + nd].copy()
        else:
            raise ValueError("Wrong input coords")
        rel = pts - np.asarray(_ref_center)[np.newaxis, :]
        shifts = np.array([np.dot(generate_polynomial_data(rel, o), c)
                           for c, o in zip(_consts, _fitting_orders)]).transpose()
        moved = pts - shifts + _drift
        if width == nd:
            return moved
        out = table.copy()
        out[:, 1:1 + nd] = moved
        return out

    return _shift_function


def _field_arguments(constants, fitting_orders, ref_center):
    """Constants, orders and centre of the three axes as ``ia3_poly_field_dev`` takes them."""
    _orders = [int(_o) for _o in np.array(fitting_orders).ravel()]
    _consts = [np.asarray(_c, dtype=np.float64).ravel() for _c in constants]
    if len(_orders) != 3 or len(_consts) != 3 or len(ref_center) < 3:
        raise ValueError("a chromatic field takes constants, fitting_orders and ref_center of the three axes z, x, y")
    for _c, _o in zip(_consts, _orders):
        if _o < 0:
            raise ValueError(f"fitting order {_o} should not be negative")
        if _o > 3:
            raise NotImplementedError(f"fitting order {_o}: the device field is built for orders 0 to 3")
        if len(_c) != L.poly_columns(_o):
            raise ValueError(f"{len(_c)} constants given for order {_o}, {L.poly_columns(_o)} expected")
    return _consts, _orders, np.asarray(ref_center, dtype=np.float64)[:3]


def chromatic_profile_from_constants(const_file_or_dict, single_im_size, dtype=np.float64):
    """The dense (3, Z, X, Y) field of a ``*_const.pkl`` (or of its dict: 'constants', 'fitting_orders', 'ref_center'),
    built in HBM from the constants instead of loaded from the ``.npy`` and uploaded: a ``DeviceBuffer`` for
    ``correct_fov_image(chromatic_profile={channel: buffer})``.  float64 holds what the generator saves; float32 the same
    values rounded once."""
    if isinstance(const_file_or_dict, dict):
        _info = const_file_or_dict
    elif isinstance(const_file_or_dict, str):
        with open(const_file_or_dict, 'rb') as _f:
            _info = pickle.load(_f)
    else:
        raise TypeError("Wrong input chromatic_const_file")
    _consts, _orders, _center = _field_arguments(_info['constants'], _info['fitting_orders'], _info['ref_center'])
    _shape = tuple(int(_d) for _d in single_im_size)
    if len(_shape) != 3:
        raise ValueError("single_im_size should be (Z, X, Y)")
    return DeviceBuffer.adopt(L.poly_field(_consts, _orders, _center, _shape, dtype), (3,) + _shape, dtype)


def Generate_chromatic_abbrevation(chromatic_folder, ref_folder,
                                   chromatic_channel,
                                   ref_channel=_chromatic_ref_channel,
                                   drift_channel=_drift_channel,
                                   parallel=True, num_threads=12,
                                   start_fov=0, num_images=40,
                                   correction_args={'correction_folder': _correction_folder,
                                                    'single_im_size': _image_size,
                                                    'all_channels': _allowed_colors,
                                                    },
                                   drift_args={},
                                   fitting_args={},
                                   matching_args={},
                                   crop_size=9, rsq_th=0.9,
                                   fitting_orders=1, ref_center=None,
                                   make_plots=True, save_plots=True,
                                   save_folder=None,
                                   save_name='chromatic_correction',
                                   overwrite_temp=False, overwrite_profile=False,
                                   verbose=True,
                                   ):
    """chromatic.py:119-317 — chromatic profile of ``chromatic_channel`` against ``ref_channel`` from the movies whose
    names both folders hold: returns ``(profiles, constants)``, three float64 (Z, X, Y) shift maps and the polynomial
    constants per axis.

    ``parallel`` / ``num_threads`` are accepted; the movies go through the device one after the other in this process.
    As in the reference, ``<save_name>_<ch>_<ref>_<Z>_<X>_<Y>.npy`` and ``..._const.pkl`` are written only when
    ``verbose`` is set (the saving lines :292-303 sit under ``if verbose:``); an existing pair of files is loaded instead
    of computed unless ``overwrite_profile``.  Figures go through matplotlib's Agg backend, are saved when
    ``save_plots`` is set and are never shown."""
    ## 0. inputs
    _correction_args = {_k: _v for _k, _v in _chromatic_default_correction_args.items()}
    _correction_args.update(correction_args)
    if 'illumination_profile' not in _correction_args:
        from ..io_tools.load import load_correction_profile
        _correction_args['illumination_profile'] = \
            load_correction_profile('illumination',
                                    corr_channels=[str(ref_channel), str(chromatic_channel), str(_drift_channel)],
                                    correction_folder=_correction_args['correction_folder'],
                                    all_channels=_correction_args['all_channels'],
                                    ref_channel=ref_channel,
                                    im_size=_correction_args['single_im_size'],
                                    verbose=verbose)
    _drift_args = {_k: _v for _k, _v in _chromatic_default_drift_args.items()}
    _drift_args.update(drift_args)
    _fitting_args = {_k: _v for _k, _v in _chromatic_default_fitting_args.items()}
    _fitting_args.update(fitting_args)

    ## 1. savefiles
    if save_folder is None:
        save_folder = chromatic_folder
    filename_base = save_name + '_' + str(chromatic_channel) + '_' + str(ref_channel)
    for _d in _correction_args['single_im_size']:
        filename_base += f'_{int(_d)}'
    saved_profile_filename = os.path.join(save_folder, filename_base + '.npy')
    saved_const_filename = os.path.join(save_folder, filename_base + '_const.pkl')
    if os.path.isfile(saved_profile_filename) and os.path.isfile(saved_const_filename) and not overwrite_profile:
        if verbose:
            print("+ chromatic abbrevation profiles already exists. direct load profiles")
        _ca_profiles = np.load(saved_profile_filename, allow_pickle=True)
        _const_infos = np.load(saved_const_filename, allow_pickle=True)
        _ca_constants = _const_infos['constants']
        _ca_rsqs = _const_infos['rsquares']
    else:
        ## 2. select matched fovs
        fov_names = [_fl for _fl in os.listdir(chromatic_folder) if _fl.split('.')[-1] == 'dax']
        ref_fov_names = [_fl for _fl in os.listdir(ref_folder) if _fl.split('.')[-1] == 'dax']
        sel_fov_names = [_fl for _fl in sorted(fov_names, key=lambda v: int(v.split('.dax')[0].split('_')[-1]))
                         if _fl in ref_fov_names]
        sel_fov_names = sel_fov_names[int(start_fov):int(start_fov) + int(num_images)]
        ## 3. / 4. one movie pair after the other
        if verbose:
            print(f"++ generating chromatic info for {len(sel_fov_names)} images in", end=' ')
            _multi_start = time.time()
        spot_infos = [find_chromatic_spot_pairs(os.path.join(chromatic_folder, _fov), os.path.join(ref_folder, _fov),
                                                chromatic_channel, ref_channel, drift_channel,
                                                _correction_args, _drift_args, _fitting_args, matching_args,
                                                crop_size, rsq_th, True, None, overwrite_temp, verbose)
                      for _fov in sel_fov_names]
        if verbose:
            print(f"{time.time()-_multi_start:.3f}s.")
        ## 5. summarize spots from multiple fovs
        _shift_dists = []
        _ref_coords = []
        for _infos in spot_infos:
            for _info in _infos:
                _shift_dists.append(_info['ca_coord'] + _info['drift'] - _info['ref_coord'])
                _ref_coords.append((_info['ref_coord'] + _info['ca_coord']) / 2)
        _shift_dists = np.array(_shift_dists)
        _ref_coords = np.array(_ref_coords)
        if ref_center is None:
            _ref_center = np.array(_correction_args['single_im_size'])[:np.shape(_ref_coords)[1]] / 2
        else:
            _ref_center = np.array(ref_center)[:np.shape(_ref_coords)[1]]
        _ref_coords = _ref_coords - _ref_center[np.newaxis, :]
        ## 6. do ploynomial fitting
        import scipy.linalg
        _dim = np.shape(_shift_dists)[1]
        if isinstance(fitting_orders, int) or isinstance(fitting_orders, np.int32):
            _fitting_orders = np.ones(_dim, dtype=np.int32) * int(fitting_orders)
        elif isinstance(fitting_orders, list) or isinstance(fitting_orders, np.ndarray):
            _fitting_orders = np.array(fitting_orders)[:_dim]
        else:
            raise TypeError("Wrong input type for fitting_orders")
        if verbose:
            print(f"++ fitting polynomial orders: {_fitting_orders}")
        _ca_constants = []
        _ca_rsqs = []
        for _i, _max_order in enumerate(_fitting_orders):
            _X = generate_polynomial_data(_ref_coords, _max_order)
            _y = _shift_dists[:, _i]
            _C, _r, _r2, _r3 = scipy.linalg.lstsq(_X, _y)
            _rsquare = 1 - np.sum((_X.dot(_C) - _y)**2) / np.sum((_y - np.mean(_y))**2)   # r2 = 1 - SSR/SST
            if verbose:
                print(f"-- constants: {_C} with rsquare={_rsquare}")
            _ca_constants.append(_C)
            _ca_rsqs.append(_rsquare)
        # the three dense profiles (:282-289) on the device, downloaded once
        _buf = chromatic_profile_from_constants({'constants': _ca_constants, 'fitting_orders': _fitting_orders,
                                                 'ref_center': _ref_center},
                                                _correction_args['single_im_size'], np.float64)
        try:
            _ca_profiles = list(_buf.download())
        finally:
            _buf.free()
        ## 7. save profiles and constants (only when verbose, as the reference)
        if verbose:
            print(f"++ saving new profiles into folder: {save_folder}")
            np.save(saved_profile_filename.replace('.npy', ''), _ca_profiles)
            _const_dict = {
                'fitting_orders': _fitting_orders,
                'constants': _ca_constants,
                'rsquares': _ca_rsqs,
                'ref_center': _ref_center,
            }
            with open(saved_const_filename, 'wb') as _f:
                pickle.dump(_const_dict, _f)
    ## 8. plots
    if make_plots:
        _plot_chromatic(_ca_profiles, _ca_rsqs, saved_profile_filename, save_plots, verbose)
    return _ca_profiles, _ca_constants


def _plot_chromatic(profiles, rsqs, profile_filename, save_plots, verbose):
    """The figures of chromatic.py:306-315 through the Agg backend: ``<profile>_<axis>.png`` when ``save_plots``."""
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except Exception as _e:
        if verbose:
            print(f"-- make_plots: matplotlib is not available ({_e}), no figure is drawn")
        return
    for _i, (_pf, _rsq) in enumerate(zip(profiles, rsqs)):
        _fig = plt.figure(dpi=150, figsize=(4, 3))
        plt.imshow(_pf.mean(tuple(np.arange(len(np.shape(_pf)) - 2))))
        plt.colorbar()
        plt.title(f"shift axis {_i}, rsq={_rsq:.3f}")
        if save_plots:
            _fig.savefig(profile_filename.replace('.npy', f'_{_i}.png'), transparent=True)
        plt.close(_fig)


def find_chromatic_spot_pairs(ca_filename: str,
                              ref_filename: str,
                              ca_channel: str,
                              ref_channel='647', drift_channel='488',
                              correction_args={},
                              drift_args={},
                              fitting_args={},
                              matching_args={},
                              crop_size=9, rsq_th=0.9,
                              save_temp=True, save_name=None,
                              overwrite=False, verbose=True,
                              ):
    """chromatic.py:322-412 — matched spot pairs of one chromatic movie and its reference movie: a list of dicts with
    'ref_coord', 'ca_coord' (float32 rows of ``find_paired_centers``), 'drift', 'ref_im', 'ca_im' (uint16 boxes of
    ``crop_size``), 'rsquare', 'slope' (float64, shape (1,)), 'intercept' (np.float64), 'ca_file', 'ref_file', for the
    pairs whose boxes regress on each other with ``rsquare >= rsq_th``.

    Both images stay resident from ``correct_fov_image`` through the fits; all boxes and regressions of the movie come
    from one ``ia3_crop_pairs_dev`` call.  The temp file ``chromatic_<movie>_channel_<ca>_ref_<ref>.pkl`` beside the movie
    is read when it exists (unless ``overwrite``) and written when ``save_temp``."""
    _basename = os.path.basename(ca_filename).replace('.dax', f'_channel_{ca_channel}_ref_{ref_channel}.pkl')
    _basename = 'chromatic_' + _basename
    temp_filename = os.path.join(os.path.dirname(ca_filename), _basename)
    if os.path.isfile(temp_filename) and not overwrite:
        if verbose:
            print(f"-- directly load from temp_file:{temp_filename}")
        with open(temp_filename, 'rb') as _f:
            _infos = pickle.load(_f)
    else:
        _held = []
        try:
            # reference image and its beads
            _ref_ims = correct_fov_image(ref_filename,
                                         [ref_channel, drift_channel],
                                         **correction_args, **drift_args,
                                         calculate_drift=False,
                                         warp_image=False,
                                         return_drift=False,
                                         verbose=verbose, return_device=True)[0]
            _held += list(_ref_ims)
            # chromatic image, drift against the reference beads
            # (the reference unpacks three values here, :361; correct_fov_image returns the drift flag as a fourth)
            _ca_out = correct_fov_image(ca_filename,
                                        [ca_channel, drift_channel],
                                        **correction_args,
                                        **drift_args,
                                        ref_filename=_ref_ims[1],
                                        calculate_drift=True,
                                        warp_image=False,
                                        return_drift=True,
                                        verbose=verbose, return_device=True)
            _ca_ims, _drift = _ca_out[0], _ca_out[2]
            _held += list(_ca_ims)
            _ref_spots = fit_fov_image(_ref_ims[0], ref_channel, **fitting_args, verbose=verbose)
            _ca_spots = fit_fov_image(_ca_ims[0], ca_channel, **fitting_args, verbose=verbose)
            _new_dft, _ca_cts, _ref_cts = find_paired_centers(_ca_spots, _ref_spots, -_drift,
                                                              **matching_args, return_paired_cts=True)
            _infos = []
            if len(_ca_cts) > 0:
                # x = the reference box, y = the chromatic box (:387-390)
                _rims, _cims, (_slopes, _intercepts, _rsqs) = L.crop_pairs(
                    _ref_ims[0], _ref_cts, _box_sizes(crop_size), _ca_ims[0], _ca_cts, regress=True)
                for _k, (_ca_ct, _ref_ct) in enumerate(zip(_ca_cts, _ref_cts)):
                    if _rsqs[_k] >= rsq_th:
                        _infos.append({
                            'ref_coord': _ref_ct,
                            'ca_coord': _ca_ct,
                            'drift': _drift,
                            'ref_im': _rims[_k].copy(),
                            'ca_im': _cims[_k].copy(),
                            'rsquare': float(_rsqs[_k]),
                            'slope': np.array([_slopes[_k]], dtype=np.float64),
                            'intercept': np.float64(_intercepts[_k]),
                            'ca_file': ca_filename,
                            'ref_file': ref_filename,
                        })
        finally:
            for _im in _held:
                if isinstance(_im, L.DeviceStack):
                    _im.free()
        if save_temp:
            if verbose:
                print(f"--- saving {len(_infos)} points to file:{temp_filename}")
            with open(temp_filename, 'wb') as _f:
                pickle.dump(_infos, _f)
    return _infos
