"""Fixtures of chromosome selection by candidate spots: tests/golden/select.npz.

Runs the reference's own ``select_candidate_chromosomes`` (segmentation_tools/chromosome.py:363-406) and
``assign_spots_to_chromosomes`` (spot_tools/picking.py:767-794) on the cases of tests/harness/select_cases.py.  The two
modules are loaded file by file as oracle/ref_loader.py loads the others; stand-ins for what picking.py imports and this
path never calls: ``tqdm``, ``spot_tools.scoring`` and ``spot_tools.checking`` (empty modules).  Only outputs are stored:
per case the kept coordinates, the captured ``_verbose`` output, whether ``max()`` of the emptied list raised, and the
assignment of round 0's selected spots to the candidates as index arrays (row ids per chromosome, concatenated, with the
count per chromosome).  Needs the reference tree (IA3_REFERENCE); nothing here runs on the GPU.

    python scripts/make_select_golden.py

The script asserts what the tests rely on: that tests/harness/select_ref.py (the literal loop and the incremental form)
reproduces every stored array byte for byte, and the printed text.
"""
import contextlib
import io
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

OUT = os.path.join(ROOT, "tests", "golden")


def load_modules():
    """The reference's (segmentation_tools/chromosome.py, spot_tools/picking.py) with the stand-ins above."""
    import ref_loader
    ns = ref_loader.load_reference()
    st = sys.modules["IA3.spot_tools"]
    for name in ("scoring", "checking"):
        m = types.ModuleType("IA3.spot_tools." + name)
        sys.modules[m.__name__] = m
        setattr(st, name, m)
    if "tqdm" not in sys.modules:
        try:
            import tqdm  # noqa: F401
        except ImportError:
            sys.modules["tqdm"] = types.ModuleType("tqdm")
            sys.modules["tqdm"].tqdm = lambda it, *a, **k: it
    picking = ns._load("IA3.spot_tools.picking", ref_loader.REF + "/spot_tools/picking.py")
    st.picking = picking
    if "IA3.segmentation_tools" not in sys.modules:
        seg = types.ModuleType("IA3.segmentation_tools")
        seg.__path__ = []
        sys.modules["IA3.segmentation_tools"] = seg
    chromosome = ns._load("IA3.segmentation_tools.chromosome", ref_loader.REF + "/segmentation_tools/chromosome.py")
    return chromosome, picking


def main():
    from harness import select_cases as K
    from harness import select_ref as R
    chromosome, picking = load_modules()
    assert list(picking._distance_zxy) == list(R.DISTANCE_ZXY) == list(K.DISTANCE_ZXY)
    d = {}
    for name in K.CASES:
        cands, spots_list, int_th, loss_th = K.case(name)
        buf, raised, kept = io.StringIO(), False, np.zeros((0, 3))
        with contextlib.redirect_stdout(buf):
            try:
                kept = chromosome.select_candidate_chromosomes(cands, spots_list, _cand_spot_intensity_th=int_th,
                                                               _good_chr_loss_th=loss_th, _verbose=True)
            except ValueError as e:
                assert "empty sequence" in str(e), e
                raised = True
        assert raised == (name in K.RAISES), name
        inc, lit = R.incremental(cands, spots_list, int_th, loss_th), R.literal(cands, spots_list, int_th, loss_th)
        for rec in (inc, lit):
            assert rec["raised"] == raised and rec["text"] == buf.getvalue(), (name, rec["text"], buf.getvalue())
            if not raised:
                assert rec["coords"].dtype == kept.dtype and rec["coords"].tobytes() == kept.tobytes(), name
        d[name + "_kept"], d[name + "_text"], d[name + "_raised"] = kept, np.array(buf.getvalue()), np.array(raised)
        # the assignment of round 0 to all candidates
        _spots = np.array(spots_list[0])
        sel = _spots[_spots[:, 0] >= int_th]
        lists = picking.assign_spots_to_chromosomes(sel, cands)
        ids = [np.asarray(np.asarray(rows).reshape(-1, 5)[:, 4], dtype=np.int64) for rows in lists]
        want = R.assign(sel, cands)
        assert len(ids) == len(want) and all(np.array_equal(sel[w, 4].astype(np.int64), i) for w, i in zip(want, ids)), name
        d[name + "_assign_ids"] = np.concatenate(ids) if ids else np.zeros(0, dtype=np.int64)
        d[name + "_assign_counts"] = np.array([len(i) for i in ids], dtype=np.int64)
        print(name, "candidates", len(cands), "kept", len(kept), "raised", raised)
    d["source"] = np.array("reference")
    path = os.path.join(OUT, "select.npz")
    np.savez_compressed(path, **d)
    print("arrays", len(d), "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
