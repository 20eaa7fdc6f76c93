"""GPU: the fit kernel (csrc/fit.hip) off its default options — ball radii 1-4, first-fit and refit centre bounds swapped,
equal and larger than the ball, width maps off 0.5 / 4 / 1.5, convergence bounds and sweep limits that cut the loop short,
the legacy model at radius 4 — against the oracle's rows, bit for bit between the driver's modes, between ia3_fit_run and
ia3_fit_first + ia3_fit_repeat, and through the Python classes.

Every input comes from tests/harness/fitopt_cases.py, whose gate (tests/test_fit_options_cpu.py) admits a case on the
reference alone.  Tolerances are tests/test_gpu_fit_pair.py's (assert_rows; test_legacy_model_pair's for the legacy model),
unchanged."""
import ctypes as C

import numpy as np
import pytest

from harness import fitopt_cases as FC
from test_gpu_fit_pair import RTOL, assert_rows, run_fit, three_ways

pytestmark = pytest.mark.gpu

IDS = [c["name"] for c in FC.SMALL]


@pytest.fixture(scope="module")
def L():
    from imageanalysis3_amd import _lib
    _lib.check(_lib.lib().ia3_init(0))
    return _lib


def params_of(L, case):
    return L.make_fit_params(model_variant=1 if case["legacy"] else 0, **case["opt"])


def assert_case_rows(case, ps, o):
    if not case["legacy"]:
        return assert_rows(ps, o["rows"])
    ref = o["rows"]          # tolerances of test_legacy_model_pair
    assert not np.isnan(ps).any() and not np.isnan(ref).any()
    np.testing.assert_allclose(ps[:, :8], ref[:, :8], rtol=RTOL, atol=1e-4)
    np.testing.assert_allclose(ps[:, 8:], ref[:, 8:], rtol=1e-3, atol=2e-3)


def same(a, b, what):
    """two results of run_fit: tables bit for bit (NaN rows by their bit pattern), fit, evaluation and sweep counts"""
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), (what, a[0], b[0])
    assert a[1:] == b[1:], (what, a[1:], b[1:])


def with_tuning(L, knob, value, fn):
    lib = L.lib()
    try:
        L.check(lib.ia3_set_tuning(knob, value))
        return fn()
    finally:
        L.check(lib.ia3_set_tuning(knob, 1))


def split_fit(L, im, seeds, fp):
    """ia3_fit_first, then ia3_fit_repeat: (rows, fits, nfev, n_iter of the repeat call), the voxel counts of the first
    fit and n_iter as ia3_fit_results_ex reports it"""
    lib = L.lib()
    seeds = np.ascontiguousarray(seeds, dtype=np.float64)
    n = len(seeds)
    st = L.DeviceStack.upload(im)
    try:
        hh = C.c_void_p()
        L.check(lib.ia3_fit_create(st._h, L.dptr(seeds), n, C.byref(fp), C.byref(hh)))
        try:
            L.check(lib.ia3_fit_first(hh))
            nvox = np.empty(n, np.int32)
            first = np.empty((n, 11), np.float32)
            L.check(lib.ia3_fit_results(hh, L.ptr(first), None, L.ptr(nvox)))
            it = C.c_int(-1)
            L.check(lib.ia3_fit_repeat(hh, C.byref(it)))
            ps = np.empty((n, 11), np.float32)
            it2 = C.c_int(-1)
            L.check(lib.ia3_fit_results_ex(hh, L.ptr(ps), None, None, C.byref(it2)))
            a, b = C.c_int64(0), C.c_int64(0)
            L.check(lib.ia3_fit_stats(hh, C.byref(a), C.byref(b)))
        finally:
            lib.ia3_fit_destroy(hh)
    finally:
        st.free()
    return (ps, a.value, b.value, it.value), first, nvox, it2.value


# ---- every case: oracle rows, driver modes, split calls ----------------------------------------------------------------
@pytest.mark.parametrize("case", FC.SMALL, ids=IDS)
def test_rows_equal_oracle_in_every_driver_mode(L, case):
    im, seeds = FC.stack_of(case)
    o = FC.oracle(case)
    fp = params_of(L, case)
    got = three_ways(L, im, seeds, fp=fp)            # IA3_TUNE_FIT_PAIR 0/1, IA3_TUNE_FIT_FUSE 0/1
    ps, fits, nfev, sweeps = got
    print(case["name"], "fits", fits, "nfev", nfev, "sweeps", sweeps, "| oracle fits", o["fits"], "nfev", o["nfev"],
          "n_iter", o["n_iter"], "| rel %.3g abs %.3g" % FC.row_gap(ps.astype(np.float64), o["rows"]))
    assert_case_rows(case, ps, o)
    assert sweeps == o["n_iter"]
    same(with_tuning(L, L.IA3_TUNE_FIT_MERGE, 0, lambda: run_fit(L, im, seeds, fp)), got, "merge 0")
    # IA3_TUNE_FIT_MEMO: tables and sweep counts bit for bit; its counters count the fits that ran (include/ia3.h), so with
    # the memo off they are every fit the reference runs, with it on never more
    nomemo = with_tuning(L, L.IA3_TUNE_FIT_MEMO, 0, lambda: run_fit(L, im, seeds, fp))
    print(case["name"], "memo 0: fits", nomemo[1], "nfev", nomemo[2])
    assert np.array_equal(nomemo[0].view(np.uint32), ps.view(np.uint32)) and nomemo[3] == sweeps
    assert nomemo[1] == o["fits"] and fits <= nomemo[1] and nfev <= nomemo[2]


@pytest.mark.parametrize("case", FC.SMALL, ids=IDS)
def test_first_then_repeat_equals_run(L, case):
    im, seeds = FC.stack_of(case)
    o = FC.oracle(case)
    fp = params_of(L, case)
    whole = run_fit(L, im, seeds, fp)
    split, first, nvox, n_iter = split_fit(L, im, seeds, fp)
    assert np.array_equal(split[0].view(np.uint32), whole[0].view(np.uint32))
    assert split[3] == n_iter == whole[3] == o["n_iter"]
    assert np.array_equal(nvox, o["nvox"])
    if case["legacy"]:
        np.testing.assert_allclose(first[:, :8], o["first"][:, :8], rtol=RTOL, atol=1e-4)
        np.testing.assert_allclose(first[:, 8:], o["first"][:, 8:], rtol=1e-3, atol=2e-3)
    else:
        assert_rows(first, o["first"])


@pytest.mark.parametrize("n_max_iter", [-1, -5])
def test_negative_sweep_limit_runs_the_one_sweep_of_the_reference(L, n_max_iter):
    """the reference tests n_iter > n_max_iter after a sweep: a negative limit gives one sweep, not the first fit's rows"""
    case = FC.BY_NAME["n_max_iter_%d-clu-f32" % n_max_iter]
    im, seeds = FC.stack_of(case)
    o = FC.oracle(case)
    assert o["n_iter"] == 1 and FC.row_gap(o["rows"], o["first"])[0] > 1e-3      # the sweep moves the rows
    ps, fits, nfev, sweeps = run_fit(L, im, seeds, params_of(L, case))
    assert sweeps == 1
    assert_rows(ps, o["rows"])
    split, first, nvox, n_iter = split_fit(L, im, seeds, params_of(L, case))
    assert split[3] == 1 and n_iter == 1 and np.array_equal(split[0].view(np.uint32), ps.view(np.uint32))


# ---- the Python classes ------------------------------------------------------------------------------------------------
def test_python_classes_pass_their_options_on(L):
    from imageanalysis3_amd.External import Fitting_v3, Fitting_v4
    for name in ("delta_2.5_1-iso-f32", "w_1_2_1.5-mild-u16", "all_off-clu-f32", "legacy-clu-f32"):
        case = FC.BY_NAME[name]
        im, seeds = FC.stack_of(case)
        cls = Fitting_v3.iter_fit_seed_points if case["legacy"] else Fitting_v4.iter_fit_seed_points
        f = cls(im, seeds.T, **case["opt"])
        split, first, nvox, n_iter = split_fit(L, im, seeds, params_of(L, case))
        f.firstfit()
        assert np.array_equal(np.array(f.ps).view(np.uint32), first.view(np.uint32)), name
        assert np.array_equal(f.nvox, nvox)
        f.repeatfit()
        assert np.array_equal(np.array(f.ps).view(np.uint32), split[0].view(np.uint32)), name
        assert f.n_iter == n_iter == FC.oracle(case)["n_iter"]
        f.release()


# ---- the host's sweep loop ---------------------------------------------------------------------------------------------
def counted(L, fn):
    """fn() and the launches of the fit kernel it made: (result, first launches, repeat launches)"""
    L.check(L.lib().ia3_sync())
    L.profile_enable(True)
    try:
        L.profile_collect()
        res = fn()
        prof = L.profile_collect()
    finally:
        L.profile_enable(False)
    return res, prof.get("fit_first", (0, 0.0))[0], prof.get("fit_repeat", (0, 0.0))[0]


@pytest.mark.parametrize("case", FC.BIG, ids=[c["name"] for c in FC.BIG])
def test_sweep_loop(L, case):
    """run_sweeps with sweep limits that cut the loop short, on fields whose cluster of four never settles at max_dist_th =
    1e-3 while every other seed does with sweep 1 (tests/test_fit_options_cpu.py::test_sweep_limits_truncate).

    ``big`` (81 seeds, four with neighbours: more than one in 64): the kernel keeps the first two stages, four unconverged
    seeds are more than one in 64, the sweeps go out in pairs, ceil((n_max_iter + 2) / 2) launches with IA3_TUNE_FIT_MERGE
    on or off.  ``dense`` (305 seeds, six with neighbours: 6 * 64 > 305, so again two stages first; then 4 * 64 <= 305):
    few_left, every remaining sweep in ONE launch; in pairs with IA3_TUNE_FIT_MERGE 0."""
    im, seeds = FC.stack_of(case)
    o = FC.oracle(case)
    n, last = len(seeds), max(case["opt"]["n_max_iter"], 0) + 2
    fp = params_of(L, case)
    got, first, repeat = counted(L, lambda: run_fit(L, im, seeds, fp))
    pairs, first0, repeat0 = counted(L, lambda: with_tuning(L, L.IA3_TUNE_FIT_MERGE, 0, lambda: run_fit(L, im, seeds, fp)))
    nomemo = with_tuning(L, L.IA3_TUNE_FIT_MEMO, 0, lambda: run_fit(L, im, seeds, fp))
    print(case["name"], "n", n, "fits", got[1], "nfev", got[2], "sweeps", got[3], "launches", first, repeat, "| pairs", pairs[1:],
          "launches", first0, repeat0, "| memo 0", nomemo[1:], "| oracle fits", o["fits"], "nfev", o["nfev"], "n_iter", o["n_iter"],
          "| rel %.3g abs %.3g" % FC.row_gap(got[0].astype(np.float64), o["rows"]))
    assert_rows(got[0], o["rows"])
    assert got[3] == o["n_iter"] == last - 1
    same(pairs, got, "merge 0")
    assert (first0, repeat0) == (1, (last + 1) // 2 - 1)
    if case["field"] == "dense":
        assert 4 * 64 <= n < 6 * 64
        assert (first, repeat) == (1, 1 if last > 2 else 0)
    else:
        assert n < 4 * 64
        assert (first, repeat) == (first0, repeat0)
    # ia3_fit_stats: without the memo every refit the reference runs and no other; with it never more
    assert np.array_equal(nomemo[0].view(np.uint32), got[0].view(np.uint32)) and nomemo[3] == got[3]
    assert nomemo[1:3] == (o["fits"], o["nfev"]) and got[1] <= o["fits"] and got[2] <= o["nfev"]


# ---- several fields ----------------------------------------------------------------------------------------------------
def test_group_fit_with_options_equals_one_by_one(L):
    """ia3_fit_fovs / ia3_fit_create_fovs on two fields with every option off its default: the per-field fitters' rows"""
    case = FC.BY_NAME["all_off-clu-f32"]
    fp = params_of(L, case)
    sp, keep = L.make_seed_params(600.0, max_num_seeds=None)
    ims = [FC.field("clu")[0], FC.field("iso")[0]]
    one = [L.fit_fovs([im], sp, fp, in_flight=1) for im in ims]
    assert all(len(t[0][0]) >= 6 for t in one)
    tabs, info = L.fit_fovs(ims, sp, fp, in_flight=2)
    for k, (t, i) in enumerate(zip(tabs, info)):
        assert np.array_equal(t.view(np.uint32), one[k][0][0].view(np.uint32)), k
        for key in ("n_seeds", "n_iter", "fits", "nfev", "voxel_evals"):
            assert i[key] == one[k][1][0][key], (k, key)
    assert info[0]["n_iter"] <= case["opt"]["n_max_iter"] + 1
    # explicit seeds: one fitter over both fields against a fitter per field
    lib = L.lib()
    seeds = [np.ascontiguousarray(FC.field(n)[1]) for n in ("clu", "iso")]
    stacks = [L.DeviceStack.upload(im) for im in ims]
    try:
        hh = C.c_void_p()
        arr_im = (C.c_void_p * 2)(*[s._h.value for s in stacks])
        arr_c = (C.c_void_p * 2)(*[s.ctypes.data for s in seeds])
        arr_n = (C.c_int * 2)(*[len(s) for s in seeds])
        L.check(lib.ia3_fit_create_fovs(arr_im, arr_c, arr_n, 2, C.byref(fp), C.byref(hh)))
        try:
            L.check(lib.ia3_fit_run(hh))
            ps = np.empty((sum(len(s) for s in seeds), 11), np.float32)
            it = C.c_int(0)
            L.check(lib.ia3_fit_results_ex(hh, L.ptr(ps), None, None, C.byref(it)))
        finally:
            lib.ia3_fit_destroy(hh)
    finally:
        for s in stacks:
            s.free()
    per = [run_fit(L, im, s, fp) for im, s in zip(ims, seeds)]
    assert np.array_equal(ps.view(np.uint32), np.concatenate([p[0] for p in per]).view(np.uint32))
    assert it.value == max(p[3] for p in per)
    assert_rows(per[0][0], FC.oracle(case)["rows"])


# ---- errors ------------------------------------------------------------------------------------------------------------
def _create_fails(L, st, seeds, fp, fovs=False):
    lib = L.lib()
    seeds = np.ascontiguousarray(seeds, dtype=np.float64)
    hh = C.c_void_p()
    if fovs:
        rc = lib.ia3_fit_create_fovs((C.c_void_p * 1)(st._h.value), (C.c_void_p * 1)(seeds.ctypes.data),
                                     (C.c_int * 1)(len(seeds)), 1, C.byref(fp), C.byref(hh))
    else:
        rc = lib.ia3_fit_create(st._h, L.dptr(seeds), len(seeds), C.byref(fp), C.byref(hh))
    assert rc != 0 and not hh.value
    return rc


def test_bad_options_are_refused_before_any_launch(L):
    """radius_fit 0 and 6 with the library's codes; widths outside the width map's domain (the reference returns NaN
    heights there) with IA3_EINVAL, from every entry that takes them; the Python classes raise; no kernel is launched"""
    from imageanalysis3_amd.External import Fitting_v3, Fitting_v4
    im, seeds = FC.field("iso")
    with L.DeviceStack.upload(im) as st:
        L.check(L.lib().ia3_sync())
        L.profile_enable(True)
        try:
            L.profile_collect()
            f = Fitting_v4.iter_fit_seed_points(st, seeds.T)
            f.firstfit()
            f.release()
            assert L.profile_collect()                    # the profile does see a fit's kernels
            assert _create_fails(L, st, seeds, L.make_fit_params(radius_fit=0)) == L.IA3_EINVAL
            assert _create_fails(L, st, seeds, L.make_fit_params(radius_fit=6)) == L.IA3_EUNSUPPORTED     # 922 voxels
            assert _create_fails(L, st, seeds, L.make_fit_params(radius_fit=6), fovs=True) == L.IA3_EUNSUPPORTED
            bad = [dict(min_w=0.0), dict(min_w=-0.5), dict(min_w=4.0), dict(min_w=5.0), dict(init_w=0.5), dict(init_w=0.4),
                   dict(init_w=4.0), dict(init_w=4.5), dict(min_w=1.6), dict(max_w=1.5), dict(max_w=float("nan")),
                   dict(init_w=float("nan")), dict(model_variant=1, init_w_zxy=(1.35, 1.15, 1.9), min_w=1.2),      # 1.15^2 passes the legacy range test
                   dict(model_variant=1, max_w=2.0)]       # 1.9^2 > 2.0: the legacy model starts from 1.5^2 = 2.25 >= max_w
            for kw in bad:
                for fovs in (False, True):
                    assert _create_fails(L, st, seeds, L.make_fit_params(**kw), fovs) == L.IA3_EINVAL, kw
                    assert "width" in L.lib().ia3_last_error().decode(), kw
            V3, V4 = Fitting_v3.iter_fit_seed_points, Fitting_v4.iter_fit_seed_points
            for cls, kw in ((V4, dict(radius_fit=0)), (V4, dict(radius_fit=6)), (V4, dict(init_w=0.5)), (V4, dict(min_w=4.5)),
                            (V3, dict(radius_fit=0)), (V3, dict(radius_fit=6))):
                f = cls(st, seeds.T, **kw)
                with pytest.raises((ValueError, NotImplementedError)):
                    f.firstfit()
                assert f._fitter is None
            with pytest.raises((ValueError, NotImplementedError)):             # ia3_gaussfit_voxels: the same refusal
                Fitting_v4.gaussfit_batch([np.arange(30.0)], [np.zeros((3, 30), int)], [[0, 0, 0]], init_w=4.0)
            assert not L.profile_collect()                # nothing was launched by any of them
        finally:
            L.profile_enable(False)
