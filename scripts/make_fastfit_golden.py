"""Fixtures of the Fitting_v4 fast path: tests/golden/fastfit.npz (+ fastfit.json, the calls made and the measured
np.std band).

Runs the reference's own ``normalzie_im`` / ``get_seed_points_base_v2`` / ``gfit_fast`` / ``fast_fit_big_image``
through oracle/ref_loader.py on stacks from the repo's generator (imageanalysis3_amd/synth.py).  OpenCV is not
installed, so the loader's empty ``cv2`` stand-in gets ``tests/harness/blur_ref.cv2_blur`` as its ``blur``.  Needs the
reference tree (IA3_REFERENCE); nothing here runs on the GPU.

    python scripts/make_fastfit_golden.py

The script asserts what the tests rely on: no two kept seeds of a run have equal height, no voxel lies within the
np.std tolerance band of a cutoff, and the LM rows of better_fit are all finite (no row is left out of a comparison).
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from imageanalysis3_amd import synth                # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
STD_BAND_FACTOR = 4.0      # the GPU test allows this many times the largest recorded np.std difference

# name -> (gfilt_size, filt_size, th_seed, max_num): the seed runs of each case
SEED_RUNS = {
    "c1": {"g0_f3": (0, 3, 8., None), "g0_f5": (0, 5, 8., None), "g0_f3_max3": (0, 3, 8., 3), "g5_f3": (5, 3, 6., None)},
    "c2": {"g0_f3": (0, 3, 8., None), "g5_f3": (5, 3, 6., None), "g5_f7": (5, 7, 6., None)},
    "c3": {"g0_f3": (0, 3, 8., None), "g0_f5": (0, 5, 8., None), "g5_f3": (5, 3, 6., None)},
}
# name -> keyword arguments of fast_fit_big_image
FIT_RUNS = {
    "c1": {"default": {}, "recenter": {"recenter": True}, "noavoid": {"avoid_neigbors": False}, "better": {"better_fit": True}},
    "c2": {"default": {}, "recenter": {"recenter": True}, "noavoid": {"avoid_neigbors": False}},
    "c3": {"default": {}, "recenter": {"recenter": True}},
}
# hand-placed centres of case 2, appended to its seeds: an integer pair 4 voxels apart along x (exact tie voxels), a pair
# with fractional centres, a centre whose ball the image edge cuts, a centre outside the image (a NaN row)
HAND_CENTRES_C2 = [[8., 20., 20.], [8., 24., 20.], [7.3, 30.6, 33.2], [8.9, 33.1, 35.7], [1.5, 2.2, 49.7], [-7.6, 5., 60.]]


def case1(dtype=np.float32):
    """12 x 40 x 44, five spots; two of them sit within a voxel of opposite corners, so that the brighter one removes
    the other through the wrap-around comparison alone."""
    shape = (12, 40, 44)
    centres = np.array([[0.2, 0.3, 0.2], [10.8, 38.7, 42.8], [5.4, 12.3, 30.6], [6.1, 27.8, 11.2], [4.7, 20.2, 21.9]])
    heights = np.array([3000., 4000., 2500., 3500., 5200.])
    return synth.render(shape, centres, heights, 31, dtype=dtype)


def case2():
    """16 x 48 x 52, twelve spots in two clusters."""
    shape = (16, 48, 52)
    a = np.array([[7.2, 12.4, 13.1], [8.6, 15.9, 16.4], [6.4, 10.2, 19.8], [9.3, 18.7, 11.6], [7.9, 8.3, 9.4], [5.8, 16.2, 22.3]])
    b = np.array([[8.1, 36.5, 38.2], [6.9, 39.8, 41.7], [9.4, 33.4, 43.9], [7.5, 41.3, 35.1], [8.8, 37.2, 46.6], [6.2, 32.1, 36.8]])
    heights = np.array([2600., 3100., 2200., 4100., 3600., 2900., 4700., 2400., 3300., 3900., 2700., 4400.])
    return synth.render(shape, np.concatenate([a, b]), heights, 47, dtype=np.float32)


def stacks():
    return {"c1": case1(np.float32), "c2": case2(), "c3": case1(np.uint16)}


def main():
    import ref_loader
    from harness import blur_ref
    R = ref_loader.load_reference()
    sys.modules["cv2"].blur = blur_ref.cv2_blur
    F4 = R.F4
    d, meta = {}, {"seed_runs": {}, "fit_runs": {}, "std_rel_diff": {}, "std_band_factor": STD_BAND_FACTOR}
    ims = stacks()
    cutoffs = []
    for case, im in ims.items():
        d[case + "_im"] = im
        d[case + "_norm20"] = F4.normalzie_im(im)
        for name, (g, f, th, mx) in SEED_RUNS[case].items():
            czxyh, std_ = F4.get_seed_points_base_v2(im, gfilt_size=g, filt_size=f, th_seed=th, max_num=mx)
            key = "%s_seeds_%s" % (case, name)
            d[key], d[key + "_std"] = czxyh, np.asarray(std_)
            meta["seed_runs"][key] = dict(gfilt_size=g, filt_size=f, th_seed=th, max_num=mx, n=int(czxyh.shape[1]))
            assert czxyh.shape[1] >= 2, (key, czxyh.shape)
            assert len(np.unique(czxyh[3])) == czxyh.shape[1], "equal heights in " + key
            stack = F4.normalzie_im(im, g) if g else im
            exact = np.std(stack.astype(np.float64))
            meta["std_rel_diff"][key] = float(abs(np.float64(std_) - exact) / exact)
            cutoffs.append((key, stack, np.float64(std_ * th)))
        # centres of the fit runs: the box-normalised seeds (case 2: and the hand-placed ones)
        cen = d[case + "_seeds_g5_f3"][:3].T.astype(np.float64)
        if case == "c2":
            cen = np.concatenate([cen, np.array(HAND_CENTRES_C2)])
        d[case + "_centres"] = cen
        for name, kw in FIT_RUNS[case].items():
            ps = F4.fast_fit_big_image(im, cen, verbose=False, **kw)
            key = "%s_fit_%s" % (case, name)
            d[key] = ps
            meta["fit_runs"][key] = dict(kw, n=int(len(ps)))
            if kw.get("better_fit"):
                assert ps.shape == (len(cen), 11) and np.all(np.isfinite(ps)), key
            else:
                assert ps.shape == (len(cen), 12) and ps.dtype == np.float64, (key, ps.shape, ps.dtype)
    assert np.isnan(d["c2_fit_default"][-1]).all() and np.isfinite(d["c2_fit_default"][:-1, :11]).all()
    assert F4.fast_fit_big_image(ims["c1"], np.zeros((0, 3)), verbose=False).shape == (0,)
    # the wrap-around comparison decides: voxel (0, 0, 0) of case 1 is a maximum of its in-image neighbourhood, above the
    # cutoff, and absent from the seeds (its wrapped neighbour at the far corner is brighter)
    s = d["c1_seeds_g0_f3"]
    im = ims["c1"]
    assert im[0, 0, 0] == im[:2, :2, :2].max() and im[0, 0, 0] > 8. * d["c1_seeds_g0_f3_std"]
    assert not np.any(np.all(s[:3] == 0, 0)) and np.any(np.all(s[:3].T == [11, 39, 43], 1))
    # exact tie voxels exist between the integer pair of case 2
    off = np.array(HAND_CENTRES_C2[1]) - np.array(HAND_CENTRES_C2[0])
    assert np.all(off == [0, 4, 0])
    # gfit_fast on explicit lists, with and without the reconstruction
    vals = im[3:7, 18:23, 20:24].ravel()
    X = np.array(np.meshgrid(np.arange(3, 7), np.arange(18, 23), np.arange(20, 24), indexing="ij")).reshape(3, -1)
    d["gf_vals"], d["gf_X"] = vals, X
    d["gf_plain"] = F4.gfit_fast(vals, X)
    d["gf_bk03"] = F4.gfit_fast(vals, X, bk_f=0.3)
    d["gf_recon"] = F4.gfit_fast(vals, X, reconstruct=True)
    d["gf_f64"] = F4.gfit_fast(vals.astype(np.float64), X)
    d["gf_u16"] = F4.gfit_fast(ims["c3"][3:7, 18:23, 20:24].ravel(), X)
    d["gf_empty"] = F4.gfit_fast(np.zeros(0, np.float32), np.zeros((3, 0), int))
    assert np.isnan(d["gf_empty"]).all() and np.isfinite(d["gf_recon"]).all()
    assert d["c3_fit_default"][:, 0].max() > 60000, "the uint16 wrap should show in a height"

    band = STD_BAND_FACTOR * max(meta["std_rel_diff"].values())
    meta["std_band"] = band
    for key, stack, cut in cutoffs:
        near = np.abs(stack.astype(np.float64) - cut) <= 2 * band * abs(cut) + 1e-300
        assert not near.any(), "a voxel of %s lies within the np.std band of the cutoff" % key
    np.savez_compressed(os.path.join(OUT, "fastfit.npz"), **d)
    with open(os.path.join(OUT, "fastfit.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")
    for k in sorted(meta["seed_runs"]):
        print(k, meta["seed_runs"][k], "%.3g" % meta["std_rel_diff"][k])
    print("std band", band, "bytes", os.path.getsize(os.path.join(OUT, "fastfit.npz")))


if __name__ == "__main__":
    main()
