"""Fixture of the pre-correction edge tests: tests/golden/precorr_edges.json.

Runs the reference's own functions, loaded through oracle/ref_loader.py, on the generated inputs of
tests/harness/precorr_ref.py (``CASES``) and records one CRC32 per case and output:

  hot/...            correction_tools.filter.Remove_Hot_Pixels(im, np.uint16, hot_pix_th, hot_th), ``im`` uint16 or
                     ``im.astype(np.float32)`` (the chain's call); corrections.Remove_Hot_Pixels must agree
  zshift/...         corrections.Z_Shift_Correction(im.astype(np.float32), dtype=np.uint16, normalization=False)
  illum/...          io_tools.load.correct_fov_image on a one-channel movie with only the illumination step on
  bleed/.../f32      io_tools.load.correct_fov_image on a C-channel movie with only the bleedthrough step on
  bleed/.../f64      np_oracle.bleedthrough_correction: correct_fov_image casts a profile it is handed to float32, so
                     the reference cannot be driven with a float64 mix (``sources`` in the file says which is which)
  illum_rescale/..., bleed_rescale/...
                     DaxProcesser._corr_illumination / ._corr_bleedthrough on an instance that holds the stacks

plus, under ``counts``, the candidate counts of the hot-pixel cases, the wrapping neighbour sums of the large random
field and the census of the edge quotients.  The file
holds results only.  Needs the reference tree (IA3_REFERENCE); nothing here runs on the GPU.

    python scripts/make_precorr_edge_golden.py
"""
import contextlib
import io
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import ref_loader                                   # noqa: E402
import np_oracle as O                               # noqa: E402
import conftest as T                                # noqa: E402
from harness import precorr_ref as P                # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "precorr_edges.json")


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all="ignore"):
        return fn(*a, **k)


def channel_names(n):
    return [str(900 - 50 * i) for i in range(n)]    # already in the descending order correct_fov_image sorts into


def run_correct_fov_image(load, ims, **kw):
    """The reference's correct_fov_image on a movie that interleaves ``ims``, every optional step off unless ``kw``
    turns it on."""
    names = channel_names(len(ims))
    Z, X, Y = ims[0].shape
    raw = np.zeros((Z * len(ims), X, Y), np.uint16)
    for i, im in enumerate(ims):
        raw[i::len(ims)] = im
    args = dict(single_im_size=[Z, X, Y], all_channels=names, num_buffer_frames=0, num_empty_frames=0, drift=None,
                calculate_drift=False, drift_channel=names[0], corr_channels=names, warp_image=True,
                hot_pixel_corr=False, z_shift_corr=False, illumination_corr=False, bleed_corr=False,
                chromatic_corr=False, gaussian_highpass=False, normalization=False, verbose=False)
    args.update(kw)
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "movie.dax")
        T.write_dax(path, raw)
        return quiet(load.correct_fov_image, path, names, **args)[0]


def processer(pre, ims):
    """A DaxProcesser that already holds ``ims`` (what _load_image leaves behind), without a movie file."""
    names = channel_names(len(ims))
    p = object.__new__(pre.DaxProcesser)
    p.channels, p.loaded_channels = list(names), list(names)
    p.correction_log = {c: {} for c in names}
    p.correction_folder, p.verbose = None, False
    p.image_size = np.array(ims[0].shape, dtype=np.int32)
    for c, im in zip(names, ims):
        setattr(p, "im_" + c, im.copy())
    return p, names


def main():
    R = ref_loader.load_reference()
    cor = ref_loader.load_corrections()
    load = R.io_load
    pre = sys.modules["IA3.classes.preprocess"]
    crcs, sources, counts = {}, {}, {}

    for key, spec in P.CASES.items():
        kind = spec[0]
        a = P.inputs(key)
        src = "reference"
        if kind == "hot":
            outs = [quiet(R.filter.Remove_Hot_Pixels, a[0].copy(), np.uint16, hot_pix_th=a[1], hot_th=a[2])]
            twin = quiet(cor.Remove_Hot_Pixels, a[0].copy(), np.uint16, hot_pix_th=a[1], hot_th=a[2])
            assert np.array_equal(outs[0], twin), key
            xs, ys = P.hot_candidates(a[0], a[1], a[2])
            counts[key] = dict(n_hot=int(len(xs)), n_interior=int(P.interior(xs, ys, a[0].shape).sum()))
        elif kind == "zshift":
            outs = [quiet(cor.Z_Shift_Correction, a[0].astype(np.float32), dtype=np.uint16, normalization=False)]
        elif kind == "illum":
            outs = run_correct_fov_image(load, [a[0]], illumination_corr=True,
                                         illumination_profile={channel_names(1)[0]: a[1]})
            with np.errstate(all="ignore"):
                counts[key] = P.quotient_census(a[0].astype(np.float32) / a[1][None])
        elif kind == "bleed":
            if a[1].dtype == np.float32:
                outs = run_correct_fov_image(load, a[0], bleed_corr=True, bleed_profile=a[1])
            else:
                src = "np_oracle"
                outs = quiet(O.bleedthrough_correction, a[0], a[1])
        elif kind == "illum_rescale":
            p, names = processer(pre, [a[0]])
            quiet(p._corr_illumination, correction_pf={names[0]: a[1]}, rescale=a[2])
            outs = [getattr(p, "im_" + names[0])]
        elif kind == "bleed_rescale":
            p, names = processer(pre, a[0])
            quiet(p._corr_bleedthrough, correction_pf=a[1], rescale=a[2])
            outs = [getattr(p, "im_" + c) for c in names]
        else:
            raise KeyError(key)
        for o in outs:
            assert o.dtype == np.uint16, (key, o.dtype)
        crcs[key] = [P.crc(o) for o in outs]
        sources[key] = src
    counts["hot/rand_big/wrapping_sums"] = P.wrapping_sums(P.inputs("hot/rand_big/u16")[0])

    with open(OUT, "w") as f:
        json.dump(dict(crc=crcs, counts=counts, sources={k: v for k, v in sources.items() if v != "reference"}),
                  f, indent=0, sort_keys=True)
        f.write("\n")
    print(len(crcs), "cases,", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
