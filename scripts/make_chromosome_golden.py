"""Fixtures of the candidate-chromosome path: tests/golden/chromosome.npz.

Runs the reference's own ``find_candidate_chromosomes`` (segmentation_tools/chromosome.py:264-361), loaded file by file
as oracle/ref_loader.py loads the other modules, on the stacks of tests/harness/chromseg_cases.py.  scikit-image is not
installed here: a stand-in ``skimage`` in ``sys.modules`` is backed by the five statements of
tests/harness/chromseg_ref.py (ball, opening, closing, remove_small_objects, random_walker).  Only the reference's
outputs are stored (the tests build the stacks again): per case the coordinate table, and from a second pass that
records what the function handed to ``scoreatpercentile`` and ``remove_small_objects``, the threshold, the number of
objects, the kept sizes and the kept-label volume as packed bits plus the labels of its set voxels.  Needs the reference
tree (IA3_REFERENCE); nothing here runs on the GPU.

    python scripts/make_chromosome_golden.py

The script asserts what the tests rely on: that tests/harness/chromseg_ref.py's chain reproduces every stored array, that
hole filling and closing both change voxels on the stored cases, and that the size filter removes objects.
"""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

OUT = os.path.join(ROOT, "tests", "golden")


def load_chromosome():
    """The reference's segmentation_tools/chromosome.py with the stand-in skimage; returns (module, record dict)."""
    import ref_loader
    from harness import chromseg_ref as R
    ns = ref_loader.load_reference()
    rec = {}

    def remove_small_objects(ar, min_size=64, **kw):
        out = R.remove_small_objects(ar, min_size)
        rec["n_objects"] = int(ar.max())
        rec["kept"] = out.astype(np.uint16)
        return out

    morph = types.ModuleType("skimage.morphology")
    morph.ball, morph.opening, morph.closing = R.ball, R.opening, R.closing
    morph.remove_small_objects = remove_small_objects
    seg = types.ModuleType("skimage.segmentation")
    seg.random_walker = R.random_walker
    sk = types.ModuleType("skimage")
    sk.morphology, sk.segmentation = morph, seg
    sys.modules.update({"skimage": sk, "skimage.morphology": morph, "skimage.segmentation": seg})
    st = types.ModuleType("IA3.segmentation_tools")
    st.__path__ = []
    sys.modules.setdefault("IA3.segmentation_tools", st)
    chrom = ns._load("IA3.segmentation_tools.chromosome", ref_loader.REF + "/segmentation_tools/chromosome.py")
    import scipy.stats
    real = scipy.stats.scoreatpercentile

    def scoreatpercentile(a, per, *args, **kw):
        v = real(a, per, *args, **kw)
        rec["threshold"] = np.float64(v)
        return v

    scipy.stats.scoreatpercentile = scoreatpercentile   # the function imports it at call time (:290)
    return chrom, rec


def main():
    from harness import chromseg_cases as CC
    from harness import chromseg_ref as R
    chrom, rec = load_chromosome()
    d = {}
    fill_changed = close_changed = removed = 0
    for key, name, dt, fs, per, ms in CC.golden_cases():
        im = CC.generated(name, dt)
        before = im.copy()
        rec.clear()
        coords = chrom.find_candidate_chromosomes(im, _filt_size=fs, _binary_per_th=per, _min_label_size=ms, _num_threads=2,
                                                  _verbose=False)
        assert np.array_equal(im, before)
        kept = rec["kept"]
        ids = np.unique(kept)
        ids = ids[ids > 0]
        assert coords.shape == ((len(ids), 3) if len(ids) else (0,)) and coords.dtype == np.float64
        st = R.chain(im, fs, per, 1, ms)
        assert st["threshold"] == rec["threshold"] and type(st["threshold"]) is type(rec["threshold"]), key
        assert np.array_equal(st["kept_label"], kept) and st["n"] == rec["n_objects"], key
        assert np.array_equal(st["coords"], coords), key
        fill_changed += int((st["filled"] != st["opened"]).sum() > 0)
        close_changed += int((st["closed"] != st["filled"]).sum() > 0)
        removed += int(len(ids) < st["n"])
        bits, vals = CC.pack_labels(kept)
        d[key + "_coords"] = coords
        d[key + "_threshold"] = np.float64(rec["threshold"])
        d[key + "_n"] = np.array([rec["n_objects"], len(ids)], dtype=np.int32)
        d[key + "_sizes"] = st["sizes"]
        d[key + "_bits"], d[key + "_labels"] = bits, vals
    n = len(CC.golden_cases())
    assert fill_changed >= n // 4 and close_changed >= n // 2 and removed >= 4, (fill_changed, close_changed, removed, n)
    # _calculate_binary_center: the index > 0 rule (a voxel in plane, row or column 0 is not averaged)
    m = np.zeros((4, 5, 6), bool)
    m[0:2, 0:3, 0:4] = True
    c = chrom._calculate_binary_center(m)
    assert c.tolist() == [1.0, 1.5, 2.0] and np.array_equal(c, R.binary_center(m))
    d["center_rule"] = c
    path = os.path.join(OUT, "chromosome.npz")
    np.savez_compressed(path, **d)
    print("cases", n, "fill changed", fill_changed, "closing changed", close_changed, "size filter removed", removed)
    print("bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
