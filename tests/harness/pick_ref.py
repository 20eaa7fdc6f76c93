"""NumPy statement of the population picker (the reference's spot_tools/picking.py:1567-2342), independent of the package:
``pick_by_intensity`` (:1723-1749), ``e_step`` (:1751-1876), ``m_step`` (:1906-2013), ``difference`` (:2280-2284), ``cum_val``
(:1879-1899) and the enumeration of the search nodes that the device's log tables are indexed by.

A population is ``cand_lists[p][r]``: ``[]``, ONE 1-D row (h, z, x, y) or a (k, 4) table, in nm.  Results come in the flat
layout of the device: per (chromosome, region) in C order, per candidate in population order.

The arithmetic is written out, so that it does not depend on the BLAS of the machine it runs on:
``norm_rows``  np.linalg.norm(a, axis=1): sqrt((dz*dz + dx*dx) + dy*dy), every operation rounded on its own;
``norm_vec``   np.linalg.norm of a 1-D 3-vector (BLAS ddot): sqrt(fma(dy, dy, fma(dx, dx, dz*dz))), the fused operations
               evaluated exactly with fractions and rounded once;
``nanmean``    np.nanmean(rows, axis=0).
scripts/make_pick_golden.py asserts that all of it reproduces the reference byte for byte.
"""
import hashlib
import warnings
from fractions import Fraction

import numpy as np

KINDS = ("ct", "lc", "int")     # kind 0, 1, 2 of include/ia3.h
NITER_MAX = 15


def _fma(a, b, c):
    a, b, c = float(a), float(b), float(c)
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        return a * b + c
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def norm_vec(d):
    """np.linalg.norm of one 3-vector."""
    dz, dx, dy = (np.float64(v) for v in d)
    return np.sqrt(np.float64(_fma(dy, dy, _fma(dx, dx, dz * dz))))


def norm_rows(d):
    """np.linalg.norm(d, axis=1) of an (k, 3) table."""
    d = np.asarray(d, dtype=np.float64)
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])


def nanmean(rows):
    """np.nanmean(rows, axis=0) of a (k, c) table without the warnings; rows added one after the other."""
    rows = np.asarray(rows, dtype=np.float64)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return np.nanmean(rows, axis=0)


def nanmean_loop(rows):
    """The same, spelled out: what csrc/pick.hip does."""
    rows = np.asarray(rows, dtype=np.float64)
    s, cnt = np.zeros(rows.shape[1]), np.zeros(rows.shape[1])
    for i, r in enumerate(rows):
        x = np.where(np.isnan(r), 0.0, r)
        s = x.copy() if i == 0 else s + x
        cnt += ~np.isnan(r)
    with np.errstate(invalid="ignore", divide="ignore"):
        return s / cnt


def entry_kind(entry):
    """0 empty, 1 one 1-D row, 2 a 2-D table."""
    if len(entry) == 0:
        return 0
    return np.ndim(np.array(entry))


def window(cid, ref_ids, neighbor_len, channels=None, j=None, split=False):
    """Indices into the reference rows whose mean is the local centre of a region with id ``cid`` (:1689-1699), in the order
    in which they are added: ascending id, and with ``split`` ascending index among the region's channel."""
    ref_ids = [int(v) for v in ref_ids]
    lo, hi = max(cid - neighbor_len, min(ref_ids)), min(cid + neighbor_len + 1, max(ref_ids) + 1)
    ids = sorted(set(i for i in ref_ids if lo <= i < hi and i != cid))
    inds = [ref_ids.index(i) for i in ids]
    if split:
        if not inds:    # np.intersect1d of an empty list is float64, which does not index
            raise IndexError("arrays used as indices must be of integer (or boolean) type")
        inds = sorted(set(inds) & set(k for k, c in enumerate(channels) if c == channels[j]))
    return inds


def cum_val_mid(sorted_vals, target):
    """The last ``mid`` of :1879-1899."""
    niter, m, M = 0, 0, len(sorted_vals) - 1
    while True:
        mid = int((m + M) / 2)
        if sorted_vals[mid] < target:
            m = mid
        else:
            M = mid
        niter += 1
        if M - m < 2 or niter > NITER_MAX:
            break
    return mid


def cum_val(sorted_vals, target):
    mid = cum_val_mid(sorted_vals, target)
    return (mid if mid != 0 else 0.5) / float(len(sorted_vals))


def _mid_and_value(sorted_vals, target):
    mid = cum_val_mid(sorted_vals, target)
    return mid, (mid if mid != 0 else 0.5) / float(len(sorted_vals))


def search_nodes(n):
    """Every node that a search in ``n`` sorted values can end on or pass: array ``mids`` indexed by heap number (root 1, a
    true compare goes to 2 * node + 1), -1 for a number that no search reaches.  One level of (m, M) pairs at a time."""
    if n < 1:
        raise IndexError("index 0 is out of bounds for axis 0 with size 0")
    levels = []
    node, m, M = np.array([1], dtype=np.int64), np.array([0], dtype=np.int64), np.array([n - 1], dtype=np.int64)
    for it in range(NITER_MAX + 1):
        mid = (m + M) // 2
        levels.append((node, mid))
        if it == NITER_MAX:
            break
        # the compare is true: m = mid; false: M = mid.  A child is visited when its interval is still 2 wide.
        cn = np.concatenate([2 * node + 1, 2 * node])
        cm, cM = np.concatenate([mid, m]), np.concatenate([M, mid])
        keep = cM - cm >= 2
        node, m, M = cn[keep], cm[keep], cM[keep]
        if len(node) == 0:
            break
    size = 2 * int(levels[-1][0].max() + 1)
    size = 1 << int(size - 1).bit_length()
    mids = np.full(max(size, 2), -1, dtype=np.int64)
    for node, mid in levels:
        mids[node] = mid
    return mids


def log_tables(n):
    """(np.log(mid / n), np.log(1 - mid / n)) per heap number, mid = 0.5 where the node's mid is 0; NaN for a number that
    no search reaches."""
    mids = search_nodes(n)
    v = mids.astype(np.float64)
    v[mids == 0] = 0.5
    v = v / float(n)
    v[mids < 0] = np.nan
    with np.errstate(invalid="ignore"):
        return np.log(v), np.log(1 - v)


def search_node(sorted_vals, target):
    """(mid, heap number of the node the search ends on), as the device carries it."""
    m, M, node, it = 0, len(sorted_vals) - 1, 1, 0
    while True:
        mid, last = (m + M) // 2, node
        lt = bool(sorted_vals[mid] < target)
        if lt:
            m = mid
        else:
            M = mid
        node = 2 * node + int(lt)
        it += 1
        if M - m < 2 or it > NITER_MAX:
            break
    return mid, last


def pick_by_intensity(cand_lists):
    """(P, R, 4) picks and (P, R) int32 index of the pick in its region (-1: empty)."""
    P, R = len(cand_lists), len(cand_lists[0])
    picks, idx = np.full((P, R, 4), np.nan), np.full((P, R), -1, dtype=np.int32)
    for p, regions in enumerate(cand_lists):
        for r, entry in enumerate(regions):
            if len(entry):
                t = np.array(entry, dtype=np.float64).reshape(-1, 4)
                idx[p, r] = np.argmax(t[:, 0])
                picks[p, r] = t[idx[p, r]]
    return picks, idx


def _channel_keys(channels):
    return [str(c) for c in channels]


def e_step(picked, picked_ids, ref_rows, ref_ids, neighbor_len, channels=None, split=False, centers=None):
    """``picked``, ``ref_rows``: (P, R, 4).  dict with ``ct``, ``lc``, ``int`` ((P, R) each) and ``sorted``:
    {kind: {key: sorted non-NaN values}}, keys 'all' and, with ``split``, ``str(channel)``."""
    picked, ref_rows = np.asarray(picked, dtype=np.float64), np.asarray(ref_rows, dtype=np.float64)
    P, R = picked.shape[:2]
    ct, lc = np.full((P, R), np.nan), np.full((P, R), np.nan)
    wins = [window(int(picked_ids[j]), ref_ids, neighbor_len, channels, j, split) for j in range(R)]
    for p in range(P):
        if centers is not None and centers[p] is not None:
            c = np.asarray(centers[p], dtype=np.float64)
            ctr = {None: c[1:4] if len(c) > 3 else c}
        elif split:
            ctr = {ch: nanmean(picked[p][[k for k in range(R) if channels[k] == ch]])[1:4] for ch in set(channels)}
        else:
            ctr = {None: nanmean(picked[p])[1:4]}
        for j in range(R):
            c = ctr[None] if None in ctr else ctr[channels[j]]
            ct[p, j] = norm_vec(picked[p, j, 1:4] - c)
            w = ref_rows[p][wins[j]] if len(wins[j]) else np.zeros((0, 4))
            lctr = nanmean(w) if len(w) else np.full(4, np.nan)
            lc[p, j] = norm_vec(picked[p, j, 1:4] - lctr[1:4])
    vals = {"ct": ct, "lc": lc, "int": picked[:, :, 0].copy()}
    out = dict(vals, sorted={})
    keys = _channel_keys(channels) if channels is not None else None
    for kind in KINDS:
        d = {}
        if split:
            for key in sorted(set(keys)):
                v = vals[kind][:, [k for k in range(R) if keys[k] == key]]
                d[key] = np.sort(v[~np.isnan(v)])
            d["all"] = np.sort(np.concatenate(list(d.values())))
        else:
            d["all"] = np.sort(vals[kind][~np.isnan(vals[kind])])
        out["sorted"][kind] = d
    return out


def m_step(cand_lists, cand_ids, ref_rows, ref_ids, refs, neighbor_len, center_weight=1.0, local_weight=1.0, channels=None,
           split_int=False, split_dist=False, centers=None, dist_only=False):
    """``refs``: {kind: {key: sorted values}} as ``e_step`` gives them.  dict with ``picks`` (P, R, 4), ``sel_scores`` (P, R),
    ``pick_idx`` (P, R) int32, and per candidate ``scores`` (n), ``mids`` (n, 3) int32 (ct, lc, int; -1 for a term whose
    weight is 0) and ``cdist`` (n, 2)."""
    ref_rows = np.asarray(ref_rows, dtype=np.float64)
    P, R = len(cand_lists), len(cand_lists[0])
    picks, sel = np.full((P, R, 4), np.nan), np.full((P, R), np.nan)
    idx = np.full((P, R), -1, dtype=np.int32)
    scores, mids, cdist = [], [], []
    wins = {}
    for p, regions in enumerate(cand_lists):
        tables = [np.array(e, dtype=np.float64).reshape(-1, 4) for e in regions]
        if centers is not None and centers[p] is not None:
            c = np.asarray(centers[p], dtype=np.float64)
            c = c[1:4] if len(c) > 3 else c
            ctr = {ch: c for ch in (set(channels) if split_dist else [None])}
        elif split_dist:
            ctr = {ch: nanmean(np.concatenate([tables[k] for k in range(R) if channels[k] == ch]))[1:4] for ch in set(channels)}
        else:
            ctr = {None: nanmean(np.concatenate(tables))[1:4]}
        for j, entry in enumerate(regions):
            kind, t = entry_kind(entry), tables[j]
            if kind == 0:
                continue
            if j not in wins:
                wins[j] = window(int(cand_ids[j]), ref_ids, neighbor_len, channels, j, split_dist)
            w = ref_rows[p][wins[j]] if len(wins[j]) else np.zeros((0, 4))
            lctr = nanmean(w) if len(w) else np.full(4, np.nan)
            c = ctr[channels[j] if split_dist else None]
            if kind == 1:
                dct, dlc = np.array([norm_vec(t[0, 1:4] - c)]), np.array([norm_vec(t[0, 1:4] - lctr[1:4])])
            else:
                dct, dlc = norm_rows(t[:, 1:4] - c), norm_rows(t[:, 1:4] - lctr[np.newaxis, 1:4])
            cdist.append(np.stack([dct, dlc], axis=1))
            if dist_only:
                continue
            ki, kd = (channels[j] if split_int else "all"), (channels[j] if split_dist else "all")
            scs, ms = [], []
            for s in range(len(t)):
                m3 = [-1, -1, -1]
                m3[2], v = _mid_and_value(refs["int"][ki], t[s, 0])
                sc = np.log(v)
                if center_weight != 0:
                    m3[0], v = _mid_and_value(refs["ct"][kd], dct[s])
                    sc += center_weight * np.log(1 - v)
                if local_weight != 0:
                    m3[1], v = _mid_and_value(refs["lc"][kd], dlc[s])
                    sc += local_weight * np.log(1 - v)
                scs.append(sc)
                ms.append(m3)
            scores.append(np.array(scs, dtype=np.float64))
            mids.append(np.array(ms, dtype=np.int32).reshape(-1, 3))
            idx[p, j] = np.argmax(scs)
            picks[p, j] = t[idx[p, j]]
            sel[p, j] = np.nanmax(scs)
    cat = lambda parts, shape, dt: np.concatenate(parts) if parts else np.zeros(shape, dtype=dt)   # noqa: E731
    return dict(picks=picks, sel_scores=sel, pick_idx=idx, scores=cat(scores, (0,), np.float64),
                mids=cat(mids, (0, 3), np.int32), cdist=cat(cdist, (0, 2), np.float64))


def difference(old, new):
    """The two counts of evaluate_differences: rows that moved by less than 0.01, rows whose distance is not NaN."""
    old, new = np.asarray(old, dtype=np.float64).reshape(-1, 4), np.asarray(new, dtype=np.float64).reshape(-1, 4)
    d = norm_rows(old[:, 1:4] - new[:, 1:4])
    with np.errstate(invalid="ignore"):
        return int(np.sum(d < 0.01)), int(np.sum(~np.isnan(d)))


def same_bits(a, b):
    """Equal shapes and dtypes, NaN where the other has NaN, and the same bytes everywhere else (the sign and payload of a
    NaN are not part of any result)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind != "f":
        return a.tobytes() == b.tobytes()
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all()) and a[~na].tobytes() == b[~nb].tobytes()


def digest(a):
    """sha256 of an array's bytes with every NaN written as the one NaN (see same_bits)."""
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "f":
        a = np.where(np.isnan(a), np.nan, a)
    return hashlib.sha256(a.tobytes()).hexdigest()
