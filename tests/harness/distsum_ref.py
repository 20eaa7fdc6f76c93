"""NumPy statement of the population distance summaries (csrc/distsum.hip), pinned byte for byte against the reference's
outputs by scripts/make_distsum_golden.py:
  q        scipy's pdist / cdist before the root: (dz*dz + dx*dx) + dy*dy, every operation rounded on its own; a cis stack has
           squareform's literal 0 on the diagonal, also for a row of NaNs
  median   np.nanmedian along the stack by sorting q: the middle value's root, or (lo + hi) / 2.0 of the two middle roots
  mean     np.nanmean: the roots added in the order of n with NaN as 0, over the count (a stack of 1 x 1 matrices is a
           contiguous axis, which NumPy adds pairwise: np.add.reduce)
  counts   finite q, and q <= q* for `root <= th` (q*: harness/distsum_cases.py qstar)
and of the two summary functions' dicts on a list of cells."""
from itertools import combinations_with_replacement, permutations

import numpy as np

from . import distsum_cases as K


def q_stack(a, b=None):
    """(N, Ra, Rb) squared distances of a flat case."""
    same = b is None
    b = a if same else b
    with np.errstate(invalid="ignore", over="ignore"):
        d = a[:, :, None, :] - b[:, None, :, :]
        q = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    if same:
        i = np.arange(a.shape[1])
        q[:, i, i] = 0.0
    return q


def median(q):
    s = np.sort(q, axis=0)                      # NaNs last
    c = (~np.isnan(q)).sum(axis=0)
    lo = np.take_along_axis(s, (np.maximum(c, 1) - 1)[None] // 2, axis=0)[0]
    hi = np.take_along_axis(s, c[None] // 2, axis=0)[0]
    with np.errstate(invalid="ignore"):
        lo, hi = np.sqrt(lo), np.sqrt(hi)
        out = np.where(c % 2 == 1, lo, (lo + hi) / 2.0)
    out[c == 0] = np.nan
    return out


def mean(q):
    nan = np.isnan(q)
    with np.errstate(invalid="ignore"):
        r = np.where(nan, 0.0, np.sqrt(q))
    cnt = (~nan).sum(axis=0)
    if q.shape[1] * q.shape[2] == 1:
        s = np.add.reduce(np.ascontiguousarray(r[:, 0, 0])).reshape(1, 1)
    else:
        s = np.zeros(q.shape[1:])
        for n in range(len(q)):
            s = s + r[n]
    with np.errstate(invalid="ignore", divide="ignore"):
        return s / cnt


def counts(q, th):
    """(n_finite, n_contact) as int32 and their float64 quotient."""
    with np.errstate(invalid="ignore"):
        nf = (q < np.inf).sum(axis=0).astype(np.int32)
        nc = (q <= K.qstar(th)).sum(axis=0).astype(np.int32)
    with np.errstate(invalid="ignore", divide="ignore"):
        return nf, nc, nc.astype(np.float64) / nf.astype(np.float64)


def summarise(q, function, th):
    if function == "nanmedian":
        return median(q)
    if function == "nanmean":
        return mean(q)
    return counts(q, th)[2]


def same_bits(x, y):
    x, y = np.asarray(x), np.asarray(y)
    return x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()


def same_values(x, y):
    """Byte for byte, a NaN of any payload for a NaN."""
    x, y = np.asarray(x), np.asarray(y)
    if x.shape != y.shape or x.dtype != y.dtype:
        return False
    nx, ny = np.isnan(x), np.isnan(y)
    return bool((nx == ny).all()) and x[~nx].tobytes() == y[~ny].tobytes()


def summary_by_key(cells, c1, c2, codebook, function, th):
    """The dict of Chr2ZxysList_2_summaryDist_by_key."""
    stacks = {(c1, c2): []} if c1 != c2 else {"cis_%s" % c1: [], "trans_%s" % c1: []}
    for cell in cells:
        if c1 not in cell or c2 not in cell or cell[c1] is None or cell[c2] is None:
            continue
        if c1 != c2:
            for t1 in cell[c1]:
                for t2 in cell[c2]:
                    stacks[(c1, c2)].append(q_stack(t1[None], t2[None])[0])
        else:
            stacks["cis_%s" % c1].extend(q_stack(t[None])[0] for t in cell[c1])
            for i1, i2 in permutations(range(len(cell[c1])), 2):
                stacks["trans_%s" % c1].append(q_stack(cell[c1][i1][None], cell[c1][i2][None])[0])
    chrs = np.asarray(codebook['chr'])
    out = {}
    for key, qs in stacks.items():
        if qs:
            out[key] = summarise(np.array(qs), function, th)
        else:
            names = (key.split('_')[-1],) * 2 if isinstance(key, str) else key
            out[key] = np.full([(chrs == n).sum() for n in names], np.nan)
    return out


def summary_dict(cells, codebook, function, th):
    out = {}
    for c1, c2 in combinations_with_replacement(np.unique(np.asarray(codebook['chr'])), 2):
        out.update(summary_by_key(cells, c1, c2, codebook, function, th))
    return out
