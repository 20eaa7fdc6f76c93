"""GPU: the per-cell pickers of spot_tools/picking.py and checking.check_spot_scores against the pinned reference
(tests/golden/cell_picking.npz, see tests/harness/cell_picking_cases.py for the tie rule): indices exactly, spot rows and
scores in every bit, NaN where the reference has NaN, the reference's exception with its words where it raises.  Every call
runs twice and every cell runs alone and in one batch of all cells through the flat forms; the bytes are compared.  64
merged spots in a region work; 65, and seven chromosomes, are NotImplementedError."""
import io
from contextlib import redirect_stdout

import numpy as np
import pytest

from conftest import load_golden
from harness import cell_picking_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    return load_golden("cell_picking.npz")


@pytest.fixture(scope="module")
def NS():
    from imageanalysis3_amd.spot_tools import picking, checking
    return K.namespace(picking, checking)


def _outputs(gold, key):
    out = []
    while "%s__%d" % (key, len(out)) in gold:
        out.append(gold["%s__%d" % (key, len(out))])
    return out


def _bytes(arrays):
    return [(np.asarray(a).dtype.str, np.asarray(a).shape, np.ascontiguousarray(a).tobytes()) for a in arrays]


def _agree(got, want, key):
    assert len(got) == len(want), (key, len(got), len(want))
    for i, (a, b) in enumerate(zip(got, want)):
        if b.dtype.kind == 'U':
            assert str(a) == str(b), (key, i)
        else:
            assert a.dtype.kind == b.dtype.kind or (a.dtype.kind in 'iu' and b.dtype.kind in 'iu'), (key, i, a.dtype, b.dtype)
            assert K.same(a, b), (key, i)


_CALLS = dict(K.fixture_calls())


@pytest.mark.parametrize("key", sorted(_CALLS))
def test_reference_names_equal_the_pinned_reference(NS, gold, key):
    with np.errstate(all="ignore"), redirect_stdout(io.StringIO()):
        first = _CALLS[key](NS)
        second = _CALLS[key](NS)
    _agree(first, _outputs(gold, key), key)
    assert _bytes(first) == _bytes(second), key


def _batch():
    return [K.cell(name) for name in K.BATCH]


def test_flat_merge_and_naive_alone_and_in_a_batch(NS, gold):
    P = NS.picking
    merged = P.population_merge_spot_lists(_batch())
    naive = P.population_naive_pick_spots(_batch(), distance_zxy=K.DZXY, return_indices=True, verbose=False)
    assert _bytes(K.flat(merged)) == _bytes(K.flat(P.population_merge_spot_lists(_batch())))
    for name, m, n in zip(K.BATCH, merged, naive):
        _agree(K.pack(m), _outputs(gold, "merge_%s_d" % name), name)
        _agree(K.flat(n), _outputs(gold, "naive_%s_d" % name), name)
        alone = P.population_merge_spot_lists([K.cell(name)])[0]
        assert _bytes(alone) == _bytes(m), name
        alone = P.population_naive_pick_spots([K.cell(name)], distance_zxy=K.DZXY, return_indices=True, verbose=False)[0]
        assert _bytes(K.flat(alone)) == _bytes(K.flat(n)), name


def test_flat_dynamic_alone_and_in_a_batch(NS, gold):
    P = NS.picking
    kw = dict(distance_zxy=K.DZXY, return_indices=True, verbose=False)
    with redirect_stdout(io.StringIO()):
        batch = P.population_dynamic_pick_spots(_batch(), **kw)
        again = P.population_dynamic_pick_spots(_batch(), **kw)
        assert _bytes(K.flat(batch)) == _bytes(K.flat(again))
        for name, got in zip(K.BATCH, batch):
            _agree(K.flat(got), _outputs(gold, "dyn_%s_d" % name), name)
            alone = P.population_dynamic_pick_spots([K.cell(name)], **kw)[0]
            assert _bytes(K.flat(alone)) == _bytes(K.flat(got)), name


def test_flat_em_alone_and_in_a_batch(NS, gold):
    P = NS.picking
    kw = dict(distance_zxy=K.DZXY, verbose=False, **K.BATCH_EM_KW)
    with redirect_stdout(io.StringIO()), np.errstate(all="ignore"):
        timings = {}
        batch = P.population_EM_pick_spots(_batch(), timings=timings, **kw)
        again = P.population_EM_pick_spots(_batch(), **kw)
        assert _bytes(K.flat(batch)) == _bytes(K.flat(again))
        assert 1 <= len(timings["iterations_s"]) <= 4 and timings["upload_merge_s"] > 0
        for name, got in zip(K.BATCH, batch):
            _agree(K.flat(got), _outputs(gold, "em_%s_batch" % name), name)
            alone = P.population_EM_pick_spots([K.cell(name)], **kw)[0]
            assert _bytes(K.flat(alone)) == _bytes(K.flat(got)), name


def test_sixty_four_merged_spots_work_and_the_limits_are_refused(NS, gold):
    P = NS.picking
    from imageanalysis3_amd import _lib
    cand, ids, coords = K.cell("K64")
    merged = P.population_merge_spot_lists([(cand, ids, coords)])[0]
    assert max(len(m) for m in merged) == _lib.IA3_CELLPICK_MAX_SPOTS == 64
    assert gold["tr_K64_d_K"].max() == 64
    kw = dict(distance_zxy=K.DZXY, return_indices=True, verbose=False)
    with redirect_stdout(io.StringIO()):
        got = P.population_dynamic_pick_spots([K.cell("K64")], **kw)[0]
        _agree(K.flat(got), _outputs(gold, "dyn_K64_d"), "K64")
        c65 = K.make_cell(**K.K65)
        assert max(len(m) for m in P.population_merge_spot_lists([c65])[0]) == 65
        with pytest.raises(NotImplementedError, match="at most 64"):
            P.population_dynamic_pick_spots([K.cell("A"), K.make_cell(**K.K65)], **kw)
        with pytest.raises(NotImplementedError, match="at most 6"):
            P.population_dynamic_pick_spots([K.cell("A"), K.cell("I7")], **kw)


def test_the_em_writes_into_the_callers_lists_and_dynamic_does_not(NS, gold):
    P = NS.picking
    cand, ids, coords = K.cell("A")
    before = [[t.copy() for t in lists] for lists in cand]
    with redirect_stdout(io.StringIO()):
        P.dynamic_pick_spots_for_chromosomes(cand, ids, coords, distance_zxy=K.DZXY, intensity_th=K.TH, verbose=False)
        assert all(K.same(a, b) for la, lb in zip(cand, before) for a, b in zip(la, lb))
        P.EM_pick_spots_for_chromosomes(cand, ids, coords, distance_zxy=K.DZXY, intensity_th=K.TH, num_iters=1, verbose=False)
    assert any(len(a) != len(b) for la, lb in zip(cand, before) for a, b in zip(la, lb))
