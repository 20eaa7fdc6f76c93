"""Fixtures of the population picker: tests/golden/pick.npz.

Runs the reference's own spot_tools/picking.py:1567-2342 (``pick_spots_by_intensities``, ``generate_reference_from_population``,
``pick_spots_by_scores``, ``evaluate_differences``, with ``chromosome_center_dists``, ``local_center_dists`` and ``cum_val``
for the per-candidate values) on the cases of tests/harness/pick_cases.py.  The module is loaded as
scripts/make_select_golden.py loads it.  Every call runs with ``parallel=False``, so no process is started.  Only outputs are
stored: the E-step's distances and sorted reference arrays, per candidate the distances, the mids (recomputed from the
reference's ``cum_val``) and the scores, the picks, the two counts of the difference, the printed text (times masked) and
exception class names.  Scores and picks are stored as arrays, every other array as a sha256 digest (NaNs as one NaN) in a
JSON record per case; of the large case only the pick indices and the record.  Needs the reference
tree (IA3_REFERENCE); nothing here runs on the GPU.

    python scripts/make_pick_golden.py

The script asserts what the tests rely on: that tests/harness/pick_ref.py reproduces every stored array byte for byte
(NaNs as NaNs), that the 1-D rows of the case "one_d" get other distances than the same rows as 1 x 4 tables, and that the two best candidates of every region either share their three mids or differ in score by at
least 10^6 times the bound on what two NumPy builds' ``np.log`` can move a score by.
"""
import contextlib
import io
import json
import os
import re
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

OUT = os.path.join(ROOT, "tests", "golden")
SCORE_BOUND_ULPS = 8       # |score - score'| <= 8 * 2^-52 * |score| between two NumPy builds
MARGIN = 1e6
FULL = ("scores", "sel_scores", "picks")   # stored as arrays; every other array as a digest


def mask_times(text):
    return re.sub(r"in \d+\.\d+s", "in #s", text)


def run_case(picking, R, K, name, d):
    c = K.case(name)
    cands, ids, ch, nl = c["cands"], c["ids"], c["channels"], c["neighbor_len"]
    cw, lw, si, sd, centers = c["center_weight"], c["local_weight"], c["split_int"], c["split_dist"], c["centers"]
    P, nR = len(cands), len(ids)
    split = si or sd
    picks0 = picking.pick_spots_by_intensities(K.tables_only(cands))
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), contextlib.redirect_stderr(io.StringIO()):
        ct, lc, ints = picking.generate_reference_from_population(picks0, ids, ref_channels=ch, parallel=False, neighbor_len=nl,
                                                                  split_channels=split, verbose=True)
        sel, sel_sc, all_sc = picking.pick_spots_by_scores(
            cands, ids, ref_channels=ch, ref_hzxys_list=picks0, ref_centers=centers, ref_ct_dists=ct, ref_local_dists=lc,
            ref_ints=ints, parallel=False, neighbor_len=nl, center_weight=cw, local_weight=lw,
            split_intensity_channels=si, split_distance_channels=sd, verbose=True)
    ratio = picking.evaluate_differences(picks0, sel)
    refs = {"ct": ct, "lc": lc, "int": ints}
    # the E-step's values per (chromosome, region)
    e_ct, e_lc = np.zeros((P, nR)), np.zeros((P, nR))
    for p in range(P):
        a, b, _ = picking._generate_ref_of_chr(picks0[p], ids, picks0[p], ids, None, split, ch, nl)
        e_ct[p], e_lc[p] = np.array(a, dtype=np.float64), np.array(b, dtype=np.float64)
    # per candidate: distances, mids, scores
    cdist, mids, scores = [], [], []
    for p in range(P):
        dc = picking.chromosome_center_dists(cands[p], None if centers is None else centers[p], split_channels=sd, ref_channels=ch)
        dl = picking.local_center_dists(cands[p], ids, picks0[p], ids, neighbor_len=nl, split_channels=sd, ref_channels=ch)
        for r in range(nR):
            if len(cands[p][r]) == 0:
                continue
            t = np.array(cands[p][r], dtype=np.float64).reshape(-1, 4)
            a, b = np.atleast_1d(dc[r]), np.atleast_1d(dl[r])
            cdist.append(np.stack([a, b], axis=1))
            ki, kd = (ch[r] if si else "all"), (ch[r] if sd else "all")
            for s in range(len(t)):
                m = [-1, -1, -1]
                if cw != 0:
                    m[0] = int(round(picking.cum_val(ct[kd], a[s]) * len(ct[kd])))
                if lw != 0:
                    m[1] = int(round(picking.cum_val(lc[kd], b[s]) * len(lc[kd])))
                m[2] = int(round(picking.cum_val(ints[ki], t[s, 0]) * len(ints[ki])))
                mids.append(m)
            scores.append(np.atleast_1d(np.array(all_sc[p][r], dtype=np.float64)))
    cdist, scores = np.concatenate(cdist), np.concatenate(scores)
    mids = np.array(mids, dtype=np.int32)
    sel, sel_sc = np.array(sel, dtype=np.float64), np.array(sel_sc, dtype=np.float64)

    # the statement reproduces all of it
    S = R.same_bits
    sp, _ = R.pick_by_intensity(cands)
    assert S(sp, picks0), name
    e = R.e_step(picks0, ids, picks0, ids, nl, ch, split, None)
    assert S(e["ct"], e_ct) and S(e["lc"], e_lc) and S(e["int"], picks0[:, :, 0]), name
    for kind in R.KINDS:
        assert list(e["sorted"][kind]) == list(refs[kind]), (name, list(refs[kind]))
        for key in refs[kind]:
            assert S(e["sorted"][kind][key], refs[kind][key]), (name, kind, key)
    m = R.m_step(cands, ids, picks0, ids, e["sorted"], nl, cw, lw, ch, si, sd, centers)
    assert S(m["cdist"], cdist) and S(m["mids"], mids) and S(m["scores"], scores), name
    assert S(m["picks"], sel) and S(m["sel_scores"], sel_sc), name
    near, num = R.difference(picks0, sel)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert (np.isnan(ratio) and num == 0) or ratio == np.int64(near) / np.int64(num), name

    # margins: the picks do not depend on the last bits of np.log
    k = 0
    for p in range(P):
        for r in range(nR):
            n = len(np.array(cands[p][r]).reshape(-1, 4)) if len(cands[p][r]) else 0
            sc, mm = scores[k:k + n], mids[k:k + n]
            k += n
            if n < 2:
                continue
            order = np.argsort(-sc, kind="stable")
            a, b = order[0], order[1]
            bound = SCORE_BOUND_ULPS * 2.0 ** -52 * max(abs(sc[a]), abs(sc[b]))
            assert (mm[a] == mm[b]).all() or sc[a] - sc[b] >= MARGIN * bound, (name, p, r, sc, mm)

    # the 1-D rows take another norm than the same rows as 1 x 4 tables would: the per-entry flag shows in the results
    for (p, r) in (K.ONE_D_ROWS if name == "one_d" else ()):
        plain = R.m_step(K.tables_only(cands), ids, picks0, ids, None, nl, dist_only=True)["cdist"]
        k = K.first_row(cands, p, r)
        assert cdist[k, 0] != plain[k, 0] and cdist[k, 1] != plain[k, 1], (p, r, cdist[k], plain[k])

    # stored in full: what a test reads values of (scores for the bound, picks); of everything else a digest
    stored = dict(picks0=picks0, e_ct=e_ct, e_lc=e_lc, cdist=cdist, mids=mids, scores=scores, picks=sel, sel_scores=sel_sc)
    for kind in R.KINDS:
        for key in refs[kind]:
            stored["sorted_%s_%s" % (kind, key)] = refs[kind][key]
    meta = dict(diff=[int(near), int(num)], text=mask_times(buf.getvalue()),
                keys={kind: [str(key) for key in refs[kind]] for kind in R.KINDS},
                lengths={kind: [len(refs[kind][key]) for key in refs[kind]] for kind in R.KINDS},
                digests={key: R.digest(v) for key, v in stored.items()})
    d[name + "_meta"] = np.array(json.dumps(meta, sort_keys=True))
    d[name + "_pick_idx"] = m["pick_idx"].astype(np.int8)
    if name != "big":
        for key in FULL:
            d["%s_%s" % (name, key)] = stored[key]
    print(name, "candidates", len(scores), "near", near, "of", num)


def main():
    from make_select_golden import load_modules
    from harness import pick_cases as K
    from harness import pick_ref as R
    _, picking = load_modules()
    d = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for name in K.CASES:
            run_case(picking, R, K, name, d)
        # the path through pick_spots_by_scores' own start: brightest picks and E-step inside
        c = K.case("split_both")
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf), contextlib.redirect_stderr(io.StringIO()):
            sel, sel_sc, _ = picking.pick_spots_by_scores(
                c["cands"], c["ids"], ref_channels=c["channels"], parallel=False, neighbor_len=c["neighbor_len"],
                split_intensity_channels=True, split_distance_channels=True, verbose=True)
        assert R.same_bits(np.array(sel), d["split_both_picks"]) and R.same_bits(np.array(sel_sc), d["split_both_sel_scores"])
        d["inner_text"] = np.array(mask_times(buf.getvalue()))
        # failures that the shims mirror
        c = K.case("base")
        for tag, kw in (("unbound", dict()), ("collapse", dict(split_intensity_channels=True, collapse_regions=False,
                                                               ref_channels=K.CHANNELS3 * 3))):
            try:
                with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
                    picking.pick_spots_by_scores(K.tables_only(c["cands"]), c["ids"], parallel=False, verbose=False, **kw)
                err = "none"
            except Exception as e:   # noqa: BLE001
                err = type(e).__name__
            d["raises_" + tag] = np.array(err)
            print(tag, err)
    d["source"] = np.array("reference")
    path = os.path.join(OUT, "pick.npz")
    np.savez_compressed(path, **d)
    print("arrays", len(d), "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
