"""Fixtures of the blur-normalised FFT aligners: tests/golden/fftblur.npz (+ fftblur.json, the calls made).

Runs the reference's own ``alignment_tools.blurnorm2d`` / ``fft3d_from2d`` and ``External/Fitting_v4``'s ``blurnorm2d`` /
``fftalign_2d`` / ``fft3d_from2d`` / ``minmax`` / ``translate`` / ``closest_faster`` through oracle/ref_loader.py.
OpenCV is not installed, so the loader's empty ``cv2`` stand-in is given ``tests/harness/blur_ref.cv2_blur`` as its
``blur`` — the NumPy statement of the box filter that the device kernel implements.  Needs the reference tree
(IA3_REFERENCE); nothing here runs on the GPU.

    python scripts/make_fftblur_golden.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import ref_loader                                   # noqa: E402
from harness import blur_ref                        # noqa: E402
from imageanalysis3_amd import synth                # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
MAX_DISP = 56
AT_GBS = (0, 3, 4, 5, 9)
F4_GBS = (3, 4, 5)
UNEQUAL = (slice(0, 100), slice(10, 90))
CENTRED = dict(center=[20, -10], max_disp=8)


def helper_inputs():
    """Small inputs of the host helpers (also stored in the fixture)."""
    rng = np.random.RandomState(11)
    d = {}
    d["mm_in"] = rng.randint(100, 4000, size=(7, 9)).astype(np.uint16)
    d["tr2_in"] = rng.normal(300., 40., size=(9, 12)).astype(np.float32)
    d["tr3_in"] = rng.randint(0, 5000, size=(4, 6, 7)).astype(np.uint16)
    d["cf_pts"] = rng.uniform(0, 30, size=(12, 3))
    d["cf_xyz"] = rng.uniform(0, 30, size=(300, 3))
    return d


TRANSLATIONS_2D = ([2, -3], [-1.6, 4.4], [0, 0])
TRANSLATIONS_3D = ([1, -2, 3], [-2.5, 0.4, -20])
CLOSEST = ((3, 6), (7, 4.5))   # (ic, rsearch)


def main():
    from scipy.spatial import cKDTree
    R = ref_loader.load_reference()
    sys.modules["cv2"].blur = blur_ref.cv2_blur
    at, F4 = R.alignment_tools, R.F4
    d = {}
    calls = {"stack_pair": "tests/harness/blur_ref.bead_blob_pair(dtype)", "max_disp": MAX_DISP, "im1": "src", "im2": "ref"}

    # the box filter itself, through the reference's two blurnorm2d
    rng = np.random.RandomState(3)
    b_in = rng.normal(400., 15., size=(20, 37)).astype(np.float32)
    d["blur_in"] = b_in
    for gb in (3, 4):
        d["blur_at_gb%d" % gb] = at.blurnorm2d(b_in, gb)
        d["blur_f4_gb%d" % gb] = F4.blurnorm2d(b_in, gb)
    calls["blurnorm2d"] = "alignment_tools.blurnorm2d / Fitting_v4.blurnorm2d (blur_in, gb) for gb in (3, 4)"

    # the chain on the bead-plus-blob pair
    for tag, dtype in (("f32", np.float32), ("u16", np.uint16)):
        ref, src = blur_ref.bead_blob_pair(dtype)
        for gb in AT_GBS:
            d["at_fft3d_gb%d_%s" % (gb, tag)] = at.fft3d_from2d(src, ref, gb=gb, max_disp=MAX_DISP)
        for gb in F4_GBS:
            t, cxy, cz = F4.fft3d_from2d(src, ref, gb=gb, max_disp=MAX_DISP, return_cor=True)
            d["f4_fft3d_gb%d_%s" % (gb, tag)] = t
            d["f4_fft3d_cor_gb%d_%s" % (gb, tag)] = np.array([cxy, cz])
            assert np.array_equal(F4.fft3d_from2d(src, ref, gb=gb, max_disp=MAX_DISP), t)
    calls["at_fft3d"] = "alignment_tools.fft3d_from2d(src, ref, gb=gb, max_disp=56) for gb in %s" % (AT_GBS,)
    calls["f4_fft3d"] = "Fitting_v4.fft3d_from2d(src, ref, gb=gb, max_disp=56, return_cor=True) for gb in %s" % (F4_GBS,)

    # fftalign_2d on the z-projections of the float32 pair
    ref, src = blur_ref.bead_blob_pair(np.float32)
    p_src, p_ref = np.max(src, 0), np.max(ref, 0)
    d["proj_src"], d["proj_ref"] = p_src, p_ref
    cases = {"equal": (p_src, p_ref, {}), "unequal": (p_src, p_ref[UNEQUAL], {}), "centred": (p_src, p_ref, CENTRED)}
    for name, (a, b, kw) in cases.items():
        xt, yt, cor = F4.fftalign_2d(a, b, return_cor=True, **kw)
        assert (xt, yt) == tuple(F4.fftalign_2d(a, b, **kw))
        d["f4_align_%s" % name] = np.array([xt, yt])
        d["f4_align_cor_%s" % name] = np.array(cor)
        d["at_align_%s" % name] = np.array(at.fftalign_2d(a, b, **dict(dict(max_disp=50), **kw)))
    assert not np.array_equal(d["f4_align_unequal"], d["at_align_unequal"])
    calls["fftalign_2d"] = {"equal": "(proj_src, proj_ref)", "unequal": "(proj_src, proj_ref[:100, 10:90])",
                            "centred": "(proj_src, proj_ref, center=[20, -10], max_disp=8)",
                            "note": "Fitting_v4 defaults (max_disp=50); at_align_*: alignment_tools.fftalign_2d, max_disp=50"}

    # host helpers
    h = helper_inputs()
    d.update(h)
    d["mm_default"] = F4.minmax(h["mm_in"])
    d["mm_range"] = F4.minmax(h["mm_in"], min_=-50.5, max_=3000)
    for k, t in enumerate(TRANSLATIONS_2D):
        d["tr2_out_%d" % k] = F4.translate(h["tr2_in"], t)
    for k, t in enumerate(TRANSLATIONS_3D):
        d["tr3_out_%d" % k] = F4.translate(h["tr3_in"], t)
    tree = cKDTree(h["cf_pts"])
    for k, (ic, rs) in enumerate(CLOSEST):
        d["cf_out_%d" % k] = F4.closest_faster(h["cf_xyz"], ic, tree, rsearch=rs)
    calls["helpers"] = {"minmax": ["(mm_in)", "(mm_in, min_=-50.5, max_=3000)"], "translate_2d": list(TRANSLATIONS_2D),
                        "translate_3d": list(TRANSLATIONS_3D), "closest_faster (ic, rsearch)": list(CLOSEST)}

    # the rough shift of align_beads(fft_filt_size=5) on the first drift crop of the drift.npz bead pair
    g = dict(np.load(os.path.join(OUT, "drift.npz")))
    bref, bsrc, _, _ = synth.make_bead_pair(tuple(g["bead_shape"]), 120, 21, g["bead_true_d"])
    s = tuple(slice(*c) for c in g["crops_2"][0])
    assert tuple(g["crops_2_size"]) == tuple(g["bead_shape"])
    md = np.max(bsrc[s].shape) / 2
    assert np.array_equal(at.fft3d_from2d(bsrc[s], bref[s], gb=0, max_disp=md), g["pair_rough"])
    d["beads_rough_gb5"] = at.fft3d_from2d(bsrc[s], bref[s], gb=5, max_disp=md)
    calls["beads_rough_gb5"] = "alignment_tools.fft3d_from2d(src[crop0], ref[crop0], gb=5, max_disp=max(shape) / 2) on the drift.npz pair"

    np.savez_compressed(os.path.join(OUT, "fftblur.npz"), **d)
    with open(os.path.join(OUT, "fftblur.json"), "w") as f:
        json.dump(calls, f, indent=1, sort_keys=True)
        f.write("\n")
    for k in sorted(d):
        if d[k].size <= 6:
            print(k, d[k].tolist())


if __name__ == "__main__":
    main()
