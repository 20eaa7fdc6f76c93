"""NumPy / SciPy statement of chromosome selection by candidate spots: spot_tools/picking.py:767-794
``assign_spots_to_chromosomes`` and segmentation_tools/chromosome.py:363-406 ``select_candidate_chromosomes`` (citations
relative to the reference tree).  ``literal`` is the reference's loop, every pass over every spot; ``incremental`` is the
form csrc/select.hip runs: owners and per-round counts are made once, and a removal moves only the spots the removed
candidate owned.  Both return the same record; tests/test_select_chromosomes_cpu.py holds them against each other and
against the reference's own outputs (tests/golden/select.npz)."""
import numpy as np
from scipy.spatial.distance import cdist

DISTANCE_ZXY = [200, 108, 108]


def nearest(zxys, chrom_zxys):
    """np.argmin(cdist(zxys, chrom_zxys), axis=1) in slices of rows."""
    out = np.empty(len(zxys), dtype=np.int64)
    step = max(1, (1 << 22) // max(1, len(chrom_zxys)))
    for a in range(0, len(zxys), step):
        out[a:a + step] = np.argmin(cdist(zxys[a:a + step], chrom_zxys), axis=1)
    return out


def assign(spots, chrom_coords, distance_zxy=DISTANCE_ZXY):
    """picking.py:767-794 as row indices: per chromosome the ascending indices of its rows of ``np.array(spots)``."""
    _chrom_zxys = np.array(chrom_coords) * np.array(distance_zxy)
    _spots = np.array(spots)
    if len(_spots) == 0:
        return [np.zeros(0, dtype=np.int64) for _ in _chrom_zxys]
    flags = nearest(_spots[:, 1:4] * np.array(distance_zxy), _chrom_zxys)
    return [np.where(flags == i)[0] for i in range(len(_chrom_zxys))]


def selected(spots_list, intensity_th, distance_zxy=DISTANCE_ZXY):
    """:380-382 and picking.py:783: (selected rows per round, their scaled float64 coordinates packed, R + 1 offsets)."""
    sels, tabs, starts = [], [], [0]
    for _spots in spots_list:
        _spots = np.array(_spots)
        sel = _spots[_spots[:, 0] >= intensity_th]
        sels.append(sel)
        tabs.append(np.asarray(sel[:, 1:4] * np.array(distance_zxy), dtype=np.float64).reshape(-1, 3))
        starts.append(starts[-1] + len(sel))
    return sels, np.concatenate(tabs) if tabs else np.zeros((0, 3)), np.array(starts)


def tie_counts(cands, spots_list, intensity_th=0.5, distance_zxy=DISTANCE_ZXY):
    """(selected rows whose two smallest squared distances are equal, rows in which a candidate has a smaller squared
    distance than the winner of np.argmin: unequal sums with equal roots)."""
    chrom = np.asarray(np.array(list(cands)) * np.array(distance_zxy), dtype=np.float64)
    _, zxys, _ = selected(spots_list, intensity_th, distance_zxy)
    d = zxys[:, None, :] - chrom[None, :, :]
    sums = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    wsum = sums[np.arange(len(zxys)), nearest(zxys, chrom)]
    exact = np.ptp(np.sort(sums, axis=1)[:, :2], axis=1) == 0 if chrom.shape[0] > 1 else np.zeros(len(zxys), bool)
    return int(exact.sum()), int((sums.min(axis=1) < wsum).sum())


def _text(n_cand, loss_th, n_rounds, removed, removed_lost, raised):
    """What the reference prints with ``_verbose`` (:373, :399, :404)."""
    lines = [f"- start select from {n_cand} chromosomes with loss threshold={loss_th}"]
    alive = np.ones(n_cand, dtype=bool)
    for c, l in zip(removed, removed_lost):
        lines.append(f"-- remove chr id {int(alive[:c].sum())}, percentage of lost rounds:{np.float64(l) / n_rounds:.3f}.")
        alive[c] = False
    if not raised:
        lines.append(f"-- {int(alive.sum())} chromosomes are kept.")
    return "\n".join(lines) + "\n"


def _record(cands, loss_th, n_rounds, removed, removed_lost, lost, raised, visits, owner):
    n_cand = len(cands)
    kept = np.setdiff1d(np.arange(n_cand), np.asarray(removed, dtype=np.int64))
    lost = np.asarray(lost, dtype=np.int64).copy()
    lost[np.asarray(removed, dtype=np.int64)] = removed_lost
    return dict(kept=kept, coords=np.array([cands[i] for i in kept]).copy(), removed=np.asarray(removed, dtype=np.int64),
                removed_lost=np.asarray(removed_lost, dtype=np.int64), lost=lost, raised=raised, visits=int(visits),
                owner=owner, text=_text(n_cand, loss_th, n_rounds, removed, removed_lost, raised))


def literal(cands, spots_list, intensity_th=0.5, loss_th=0.4, max_passes=None):
    """The loop of :375-399 as it stands: every pass assigns every selected spot of every round to the candidates that are
    left, flags = np.mean of "the round gave no spot", the largest flag above the threshold goes.  ``max_passes`` stops the
    loop early (scripts/time_select_chromosomes.py: a pass over an experiment takes seconds)."""
    cands = list(cands)
    orig = list(cands)
    ids = list(range(len(cands)))                     # original index of every candidate still in the list
    flags = [1 for _ in cands]
    removed, removed_lost, raised, visits = [], [], False, 0
    lost = np.zeros(len(cands), dtype=np.int64)
    owner = None
    n_rounds, passes = len(spots_list), 0
    while True:
        if not cands:
            raised = True                             # max() arg is an empty sequence
            break
        if not max(flags) > loss_th or (max_passes is not None and passes >= max_passes):
            break
        passes += 1
        empties, owners = [[] for _ in cands], []
        for _spots in spots_list:
            _spots = np.array(_spots)
            sel = _spots[_spots[:, 0] >= intensity_th]
            rows = assign(sel, cands)
            visits += len(sel) * len(cands)
            own = np.full(len(sel), -1, dtype=np.int64)
            for i, r in enumerate(rows):
                empties[i].append(len(r) == 0)
                own[r] = ids[i]
            owners.append(own)
        owner = np.concatenate(owners) if owners else np.zeros(0, dtype=np.int64)
        with np.errstate(all="ignore"):
            flags = [np.mean(e) for e in empties]
        for i, e in zip(ids, empties):
            lost[i] = int(np.sum(e))
        if np.max(flags) > loss_th:
            k = int(np.argmax(flags))
            flags.pop(k)
            cands.pop(k)
            removed.append(ids.pop(k))
            removed_lost.append(int(lost[removed[-1]]))
    return _record(orig, loss_th, n_rounds, removed, removed_lost, lost, raised, visits, owner)


def incremental(cands, spots_list, intensity_th=0.5, loss_th=0.4, distance_zxy=DISTANCE_ZXY):
    """The same result with the work of csrc/select.hip: one assignment of every spot, ``cnt[r][c]`` spots of round r
    owned by c, ``lost[c]`` rounds with cnt 0; a removal hands the removed candidate's spots to their nearest alive
    candidate (lowest original index among equals) and changes only those counts.  ``visits`` = distances evaluated."""
    cands = list(cands)
    C, R = len(cands), len(spots_list)
    if C == 0:
        return _record(cands, loss_th, R, [], [], [], True, 0, None)
    if not 1 > loss_th or R == 0:
        return _record(cands, loss_th, R, [], [], np.zeros(C), False, 0, None)
    chrom = np.asarray(np.array(cands) * np.array(distance_zxy), dtype=np.float64)
    _, zxys, starts = selected(spots_list, intensity_th, distance_zxy)
    rnd = np.repeat(np.arange(R), np.diff(starts))
    owner = nearest(zxys, chrom) if len(zxys) else np.zeros(0, dtype=np.int64)
    visits = len(zxys) * C
    cnt = np.zeros((R, C), dtype=np.int64)
    np.add.at(cnt, (rnd, owner), 1)
    lost = (cnt == 0).sum(axis=0)
    alive = np.ones(C, dtype=bool)
    removed, removed_lost, raised = [], [], False
    while True:
        idx = np.flatnonzero(alive)
        flags = lost[idx].astype(np.float64) / R
        if not flags.max() > loss_th:
            break
        c = int(idx[np.argmax(flags)])
        removed.append(c)
        removed_lost.append(int(lost[c]))
        alive[c] = False
        idx = np.flatnonzero(alive)
        if len(idx) == 0:
            raised = True
            break
        mine = np.flatnonzero(owner == c)
        visits += len(mine) * len(idx)
        if len(mine):
            new = idx[nearest(zxys[mine], chrom[idx])]
            owner[mine] = new
            np.add.at(cnt, (rnd[mine], new), 1)
            for k in np.unique(new):
                lost[k] = (cnt[:, k] == 0).sum()
    return _record(cands, loss_th, R, removed, removed_lost, lost, raised, visits, owner)
