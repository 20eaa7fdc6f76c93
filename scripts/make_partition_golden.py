"""Fixtures of the label lookups: tests/golden/partition.npz.

Runs the reference's own ``find_coordinate_intensities``, ``Spots_Partition.spots_to_labels`` / ``spots_to_DAPI``
(classes/partition_spots.py) and ``segmentation_mask_2_bounding_box`` (segmentation_tools/cell.py) through
oracle/ref_loader.py on the label images and stacks of tests/harness/partition_cases.py.  Only spot coordinates and the
reference's outputs are stored: the tests build the images again.  Needs the reference tree (IA3_REFERENCE); nothing
here runs on the GPU.

    python scripts/make_partition_golden.py

The script asserts what the tests rely on: the column order and rounding of the reference, that the tie spot does tie
between two labels (and the smaller wins), that the background spot votes -1 at every radius, and that the NumPy
statement tests/harness/partition_ref.py reproduces every stored array.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

OUT = os.path.join(ROOT, "tests", "golden")


def main():
    import ref_loader
    from harness import partition_cases as PC
    from harness import partition_ref as PR
    cell, part = ref_loader.load_partition()
    Spots3D = part.Spots3D
    SP = part.Spots_Partition
    d = {}
    for name, lab in PC.label_cases().items():
        coords = PC.spot_coords(name, lab.shape)
        spots = Spots3D(PC.spot_table(coords))
        d[name + "_coords"] = coords
        for r in PC.FCI_RADII:
            if name == "distinct" and r == 3:
                continue
            m = part.find_coordinate_intensities(lab, spots, search_radius=r)
            assert m.shape == (len(coords), (2 * r + 1) ** 3) and m.dtype == lab.dtype
            assert np.array_equal(m, PR.gather(lab, coords, r)), (name, r)
            d["%s_fci_r%d" % (name, r)] = m
        for r in PC.VOTE_RADII:
            v = SP.spots_to_labels(lab, spots, search_radius=r, verbose=False)
            assert v.dtype == np.int32 and np.array_equal(v, PR.vote(lab, coords, r)), (name, r)
            d["%s_labels_r%d" % (name, r)] = v
        ids = np.unique(lab)
        ids = ids[ids > 0]
        bx = np.array([cell.segmentation_mask_2_bounding_box(lab, int(l)).array for l in ids])
        # the call of classes/preprocess.py:1117 hands 3 to cell_id, not to the margin: the same boxes
        assert all(np.array_equal(cell.segmentation_mask_2_bounding_box(lab == l, 3).array, b) for l, b in zip(ids[:8], bx[:8]))
        table = PR.boxes(lab)
        tight = table[ids, 1:].reshape(-1, 3, 2)
        grown = np.stack([np.maximum(tight[:, :, 0] - 1, 0), np.minimum(tight[:, :, 1] + 1, np.array(lab.shape))], axis=2)
        assert np.array_equal(grown, bx), name
        d[name + "_ids"], d[name + "_boxes"] = ids.astype(np.int32), bx.astype(np.int32)
        d[name + "_union_box"] = cell.segmentation_mask_2_bounding_box(lab, None, 2).array.astype(np.int32)
        for what in PC.SPECIAL[name]:
            k = PC.special_index(name, what, lab.shape)
            for r in PC.VOTE_RADII:
                got = d["%s_labels_r%d" % (name, r)][k]
                if what == "background":
                    assert got == -1, (name, r, got)
                elif r in (1, 3, 4):   # the tie: nine (r = 1) ... voxels of each of the labels 9 and 5
                    cube = PR.gather(lab, coords[k:k + 1], r)[0]
                    assert (cube == 9).sum() == (cube == 5).sum() > 0 and got == 5, (name, r, got)
    # rounding and column order
    lab = PC.small_labels()
    one = part.find_coordinate_intensities(lab, Spots3D(PC.spot_table(np.array([[2.5, 3.5, -0.5]]))), search_radius=1)
    want = [lab[min(max(2 + dz, 0), 4), 4 + dx, max(0 + dy, 0)] for dz in (-1, 0, 1) for dx in (-1, 0, 1) for dy in (-1, 0, 1)]
    assert one[0].tolist() == want
    # intensities
    coords = PC.spot_coords("one", PC.DAPI_SHAPE)
    spots = Spots3D(PC.spot_table(coords))
    d["dapi_coords"] = coords
    for tag, im in (("u16", PC.dapi_u16()), ("f32", PC.dapi_f32()), ("nan", PC.dapi_f32(nan=True))):
        for r in PC.DAPI_RADII:
            v = SP.spots_to_DAPI(im, spots, search_radius=r, verbose=False)
            assert v.dtype == im.dtype and v.shape == (len(coords),)
            assert np.array_equal(v, PR.cube_max(im, coords, r), equal_nan=True), (tag, r)
            d["dapi_%s_r%d" % (tag, r)] = v
    assert np.isnan(d["dapi_nan_r5"]).any() and not np.isnan(d["dapi_nan_r5"]).all()
    # empty tables
    e = Spots3D(np.zeros((0, 11)))
    assert part.find_coordinate_intensities(lab, e, search_radius=2).shape == (0, 125)
    assert SP.spots_to_labels(lab, e, verbose=False).shape == (0,)
    np.savez_compressed(os.path.join(OUT, "partition.npz"), **d)
    print({k: v.shape for k, v in d.items()})
    print("bytes", os.path.getsize(os.path.join(OUT, "partition.npz")))


if __name__ == "__main__":
    main()
