"""Median distance maps and contact probabilities of a traced population on the device (reference:
structure_tools/distance.py).  ``Chr2ZxysList_2_summaryDist_by_key`` (:12-67) stacks ``squareform(pdist(zxys))`` /
``cdist(zxys1, zxys2)`` of one chromosome pair over all cells and homolog combinations and reduces the stack with
``np.nanmedian`` (or another function) along axis 0; ``Chr2ZxysList_2_summaryDict`` (:69-122) does so for every pair of the
codebook in a process pool.  Here the coordinate tables of every chromosome copy are uploaded once
(``_lib.DistancePopulation``) and every key is one library call (``ia3_dist_summary_dev``) that never makes
the stack; the results are the reference's bit for bit.  The plotting-order helpers (:124-228) are host code.

``function`` is ``'nanmedian'``, ``'nanmean'``, this module's ``contact_prob`` or a ``functools.partial`` of it with
``contact_th``; ``axis`` is 0.  Anything else raises ``NotImplementedError``: there is no CPU fallback.

All ``file:line`` citations are relative to the reference tree.
"""
import functools
import time
import warnings
from itertools import combinations_with_replacement

import numpy as np

from .. import _lib as L

default_num_threads = 12

_SUPPORTED = ("supported: function='nanmedian', function='nanmean', structure_tools.distance.contact_prob or a "
              "functools.partial of it with contact_th, and axis=0")


def contact_prob(mat, contact_th=0.6, axis=0):
    """:231-232: ``np.sum(np.array(mat) <= contact_th, axis) / np.sum(np.isfinite(mat), axis)`` of an array-like stack,
    counted on the device with the comparison itself on the given values."""
    if axis != 0:
        raise NotImplementedError("contact_prob(axis=%r) is not built; %s" % (axis, _SUPPORTED))
    stack = np.array(mat, dtype=np.float64)
    prob, nf, nc = L.dist_contact_stack(stack, contact_th, return_counts=True)
    if ((nf == 0) & (nc == 0)).any():
        warnings.warn("invalid value encountered in divide", RuntimeWarning, stacklevel=2)
    if ((nf == 0) & (nc != 0)).any():
        warnings.warn("divide by zero encountered in divide", RuntimeWarning, stacklevel=2)
    return prob


def _parse_function(function, axis):
    """(IA3_DIST_* code, contact threshold or None); TypeError as the reference for what is neither a name nor callable."""
    if not isinstance(function, str) and not callable(function):
        raise TypeError("Wrong input type for input: function")
    if axis != 0:
        raise NotImplementedError("axis=%r is not built; %s" % (axis, _SUPPORTED))
    if isinstance(function, str):
        if function == 'nanmedian':
            return L.DIST_NANMEDIAN, None
        if function == 'nanmean':
            return L.DIST_NANMEAN, None
        raise NotImplementedError("function=%r is not built; %s" % (function, _SUPPORTED))
    if function is contact_prob:
        return L.DIST_CONTACT, 0.6
    if isinstance(function, functools.partial) and function.func is contact_prob and not function.args \
            and set(function.keywords) <= {"contact_th", "axis"} and function.keywords.get("axis", 0) == 0:
        return L.DIST_CONTACT, function.keywords.get("contact_th", 0.6)
    raise NotImplementedError("function=%r is not built; %s" % (function, _SUPPORTED))


def _expand(m):
    """For counts m per cell: (cell of every item, its number inside the cell), cell by cell."""
    start = np.cumsum(m) - m
    return np.repeat(np.arange(len(m)), m), np.arange(int(m.sum())) - np.repeat(start, m)


class _Copies(object):
    """The tables of the chromosome copies of a list of cells, numbered in the order (cell, chromosome, homolog): the copies
    of one chromosome of one cell are ``first[c][cell] + 0 .. count[c][cell] - 1`` (count 0: absent, ``None`` or empty)."""

    def __init__(self, chr_2_zxys_list, chrs):
        n = len(chr_2_zxys_list)
        self.tables = []
        self.first = {c: np.zeros(n, dtype=np.int64) for c in chrs}
        self.count = {c: np.zeros(n, dtype=np.int64) for c in chrs}
        for i, cell in enumerate(chr_2_zxys_list):
            for c in chrs:
                if c not in cell or cell[c] is None:
                    continue
                self.first[c][i] = len(self.tables)
                for zxys in cell[c]:
                    t = np.asarray(zxys, dtype=np.float64)
                    if t.ndim != 2 or t.shape[1] != 3:
                        raise ValueError("a (regions, 3) coordinate table is required for chromosome %r of cell %d, got shape %s"
                                         % (c, i, t.shape))
                    self.tables.append(t)
                self.count[c][i] = len(self.tables) - self.first[c][i]
        self.rows = np.array([len(t) for t in self.tables], dtype=np.int64)

    def pairs(self, c1, c2):
        """Per key of the pair (c1, c2), in the reference's key order: the (pairs, 2) copy numbers in the order :21-41 appends
        the matrices (cell by cell; homologs of c1 outside, of c2 inside; ``permutations`` order for trans)."""
        f1, k1, f2, k2 = self.first[c1], self.count[c1], self.first[c2], self.count[c2]
        if c1 != c2:
            cell, t = _expand(k1 * k2)
            return {(c1, c2): np.stack([f1[cell] + t // np.maximum(k2[cell], 1), f2[cell] + t % np.maximum(k2[cell], 1)], axis=1)}
        cell, t = _expand(k1)
        cis = np.stack([f1[cell] + t, f1[cell] + t], axis=1)
        cell, t = _expand(k1 * (k1 - 1))
        i1, r = t // np.maximum(k1[cell] - 1, 1), t % np.maximum(k1[cell] - 1, 1)
        trans = np.stack([f1[cell] + i1, f1[cell] + r + (r >= i1)], axis=1)
        return {"cis_%s" % c1: cis, "trans_%s" % c1: trans}

    def check_shapes(self, pairs):
        """np.nanmedian of matrices of unequal shape: NumPy's ValueError."""
        rows = self.rows[pairs]
        if (rows != rows[0]).any():
            shapes = np.unique(rows, axis=0)
            raise ValueError("setting an array element with a sequence. The requested array has an inhomogeneous shape: "
                             "the distance matrices of one key have the shapes %s" % [tuple(int(v) for v in sh) for sh in shapes])
        ra, rb = rows[0]
        if ra < 1 or rb < 1:
            raise ValueError("a chromosome copy without regions: the distance matrices of a key are %d x %d" % (ra, rb))


_WARNINGS = {L.DIST_NANMEDIAN: "All-NaN slice encountered", L.DIST_NANMEAN: "Mean of empty slice",
             L.DIST_CONTACT: "invalid value encountered in divide"}


def _chr_sizes(codebook_df):
    """:47-48: regions per chromosome name (as str) in the codebook."""
    col = np.asarray(codebook_df['chr'])
    return {str(c): np.sum(col == str(c)) for c in np.unique(col)}


def _summaries(pop, copies, keys, codebook_df, code, th):
    out = {}
    sizes = None
    for key, pairs in keys.items():
        if len(pairs) > 0:
            m = pop.summary(pairs[:, 0], pairs[:, 1], function=code, contact_th=th, same=isinstance(key, str) and key.startswith("cis_"))
            if np.isnan(m).any():
                warnings.warn(_WARNINGS[code], RuntimeWarning, stacklevel=3)
            out[key] = m
        else:
            if sizes is None:
                sizes = _chr_sizes(codebook_df)
            if isinstance(key, str):
                n = sizes[key.split('_')[-1]]
                out[key] = np.nan * np.ones([n, n])
            else:
                out[key] = np.nan * np.ones([sizes[key[0]], sizes[key[1]]])
    return out


def _checked_keys(copies, c1, c2):
    keys = copies.pairs(c1, c2)
    for pairs in keys.values():
        if len(pairs) > 0:
            copies.check_shapes(pairs)
    return keys


def Chr2ZxysList_2_summaryDist_by_key(chr_2_zxys_list, _c1, _c2, codebook_df,
                                      function='nanmedian', axis=0,
                                      verbose=False):
    """:12-67.  ``{(_c1, _c2): matrix}``, or ``{'cis_c': matrix, 'trans_c': matrix}`` when the two names are equal; a key
    without any matrix gets NaNs sized from the codebook.  Cells that lack a chromosome or hold ``None`` are skipped."""
    code, th = _parse_function(function, axis)
    chrs = [_c1] if _c1 == _c2 else [_c1, _c2]
    copies = _Copies(chr_2_zxys_list, chrs)
    keys = _checked_keys(copies, _c1, _c2)
    if not copies.tables:
        return _summaries(None, copies, keys, codebook_df, code, th)
    with L.DistancePopulation.upload(copies.tables) as pop:
        return _summaries(pop, copies, keys, codebook_df, code, th)


def Chr2ZxysList_2_summaryDict(
        chr_2_zxys_list, total_codebook,
        function='nanmedian', axis=0,
        parallel=True, num_threads=default_num_threads,
        verbose=False):
    """:69-122: every pair of the codebook's chromosomes, in ``combinations_with_replacement`` order.  The population is
    uploaded once and every key is one device call; ``parallel`` and ``num_threads`` start no process."""
    code, th = _parse_function(function, axis)
    if verbose:
        print(f"-- preparing chr_2_zxys from {len(chr_2_zxys_list)} cells", end=' ')
        _start_prepare = time.time()
    _all_chrs = np.unique(np.asarray(total_codebook['chr']))
    copies = _Copies(chr_2_zxys_list, list(_all_chrs))
    all_keys = [_checked_keys(copies, _chr1, _chr2)
                for _chr1, _chr2 in combinations_with_replacement(_all_chrs, 2)]
    if verbose:
        print(f"in {time.time()-_start_prepare:.3f}s.")
        print(f"-- summarize {len(all_keys)} inter-chr distances on the device", end=' ')
    _start_time = time.time()
    _summary_dict = {}
    if copies.tables:
        with L.DistancePopulation.upload(copies.tables) as pop:
            for keys in all_keys:
                _summary_dict.update(_summaries(pop, copies, keys, total_codebook, code, th))
    else:
        for keys in all_keys:
            _summary_dict.update(_summaries(None, copies, keys, total_codebook, code, th))
    if verbose:
        print(f"in {time.time()-_start_time:.3f}s.")
    return _summary_dict


def population_distance_summary(zxys_a, zxys_b=None, function='nanmedian', contact_th=None, return_counts=False):
    """The summary of (N, R, 3) picked coordinates that the caller holds (not a reference name): the cis map of ``zxys_a``
    (``squareform(pdist(.))`` per copy), or with ``zxys_b`` of (N, Rb, 3) the map of ``cdist(zxys_a[n], zxys_b[n])``.
    ``function``: as in ``Chr2ZxysList_2_summaryDist_by_key``; ``contact_th`` replaces the threshold of a contact function
    and is what the counts use.  ``return_counts``: also (n_finite, n_contact), int32."""
    code, th = _parse_function(function, 0)
    if contact_th is not None:
        th = contact_th
    a = np.asarray(zxys_a, dtype=np.float64)
    if a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("zxys_a should be (N, R, 3) with N, R >= 1, got %s" % (a.shape,))
    tables, N = list(a), len(a)
    if zxys_b is not None:
        b = np.asarray(zxys_b, dtype=np.float64)
        if b.ndim != 3 or b.shape[2] != 3 or b.shape[0] != N or b.shape[1] < 1:
            raise ValueError("zxys_b should be (%d, Rb, 3) with Rb >= 1, got %s" % (N, b.shape))
        tables += list(b)
    pa = np.arange(N, dtype=np.int32)
    pb = pa if zxys_b is None else pa + N
    with L.DistancePopulation.upload(tables) as pop:
        return pop.summary(pa, pb, function=code, contact_th=th, same=zxys_b is None, return_counts=return_counts)


# ---- plotting order (host) ---------------------------------------------------------------------------------------------------

def sort_chr(_chr):
    """:125-133: the sort key of a chromosome name: its number, 23 for 'X', 24 for 'Y' (any other name fails as there)."""
    try:
        return int(_chr)
    except Exception:
        named = {'X': 23, 'Y': 24}
        if _chr in named:
            return named[_chr]
        raise UnboundLocalError("local variable 'out_key' referenced before assignment")


def _sorted_chrs(codebook):
    return sorted(np.unique(codebook['chr']), key=sort_chr)


def Generate_PlotOrder(total_codebook, sel_codebook, sort_by_region=True):
    """:136-162: per chromosome (in ``sort_chr`` order) the rows of ``sel_codebook`` that hold its regions and their
    ``chr_order``; with ``sort_by_region=False`` consecutive places chromosome by chromosome instead."""
    chr_2_plot_indices, chr_2_chr_orders = {}, {}
    sel_ids = sel_codebook['id'].values
    placed = 0
    for _chr in _sorted_chrs(total_codebook):
        chr_codebook = total_codebook[total_codebook['chr'] == _chr]
        inds, orders = [], []
        for _id, _ord in zip(chr_codebook['id'].values, chr_codebook['chr_order'].values):
            if _id in sel_ids:
                inds.append(sel_codebook[sel_codebook['id'] == _id].index[0])
                orders.append(_ord)
        if not inds:
            continue
        if sort_by_region:
            chr_2_plot_indices[_chr] = np.array(inds)
            chr_2_chr_orders[_chr] = np.array(orders)
        else:
            chr_2_plot_indices[_chr] = np.arange(placed, placed + len(inds))
            chr_2_chr_orders[_chr] = np.arange(len(inds))
        placed += len(inds)
    return chr_2_plot_indices, chr_2_chr_orders


def assemble_ChrDistDict_2_Matrix(dist_dict,
                                  total_codebook, sel_codebook=None,
                                  use_cis=True, use_trans=False,
                                  sort_by_region=True):
    """:164-203: one matrix over the rows of ``sel_codebook`` from the blocks of a summary dict, with the chromosome edges
    and names of ``generate_plot_chr_edges``."""
    if sel_codebook is None:
        sel_codebook = total_codebook
    plot_inds, chr_orders = Generate_PlotOrder(total_codebook, sel_codebook, sort_by_region=sort_by_region)
    size = len(sel_codebook)
    _matrix = np.ones([size, size]) * np.nan
    chrs = _sorted_chrs(total_codebook)
    for _chr1 in chrs:
        for _chr2 in chrs:
            if _chr1 not in plot_inds or _chr2 not in plot_inds:
                continue
            rows, cols = plot_inds[_chr1][:, np.newaxis], plot_inds[_chr2]
            o1, o2 = chr_orders[_chr1].astype(np.int32), chr_orders[_chr2].astype(np.int32)
            if _chr1 == _chr2:
                if use_cis and f"cis_{_chr1}" in dist_dict:
                    _matrix[rows, cols] = dist_dict[f"cis_{_chr1}"][o1[:, np.newaxis], o2]
                elif use_trans and f"trans_{_chr1}" in dist_dict:
                    _matrix[rows, cols] = dist_dict[f"trans_{_chr1}"][o1[:, np.newaxis], o2]
            elif (_chr1, _chr2) in dist_dict:
                block = dist_dict[(_chr1, _chr2)][o1[:, np.newaxis], o2]
                _matrix[rows, cols] = block
                _matrix[plot_inds[_chr2][:, np.newaxis], plot_inds[_chr1]] = block.transpose()
            elif (_chr2, _chr1) in dist_dict:
                block = dist_dict[(_chr2, _chr1)][o2[:, np.newaxis], o1]
                _matrix[rows, cols] = block.transpose()
                _matrix[plot_inds[_chr2][:, np.newaxis], plot_inds[_chr1]] = block
    _chr_edges, _chr_names = generate_plot_chr_edges(sel_codebook, plot_inds, sort_by_region)
    return _matrix, _chr_edges, _chr_names


def generate_plot_chr_edges(sel_codebook, chr_2_plot_inds=None, sort_by_region=True):
    """:207-228: where a new chromosome starts along the rows of ``sel_codebook`` (or along the places of
    ``chr_2_plot_inds``), closed by the number of rows, and the chromosomes' names."""
    if chr_2_plot_inds is None or not isinstance(chr_2_plot_inds, dict):
        chr_2_plot_inds, _ = Generate_PlotOrder(sel_codebook, sel_codebook, sort_by_region=sort_by_region)
    _chr_edges, _chr_names = [], []
    if sort_by_region:
        previous = None
        for _ind, _chr in zip(sel_codebook.index, sel_codebook['chr']):
            if _chr != previous:
                _chr_edges.append(_ind)
                _chr_names.append(_chr)
            previous = _chr
    else:
        for _chr, _inds in chr_2_plot_inds.items():
            _chr_edges.append(_inds[0])
            _chr_names.append(_chr)
    _chr_edges.append(len(sel_codebook))
    return np.array(_chr_edges), _chr_names
