"""CPU: the case table of the fitter's option tests (tests/harness/fitopt_cases.py) — every case is admitted by the gate
(a)-(d) and every option set changes what the reference computes.  The reference (oracle/np_oracle.py) and the host build of the
LM core (tests/native/lm_cpu.cpp) alone: this is also the CPU check of the LM core's width and centre maps off
min_w = 0.5, max_w = 4, init_w = 1.5 and delta = 1.0 (gate (a) runs it at every case's options).

The last test prints the worst gate values over the table; they are copied into the harness's docstring."""
import warnings

import numpy as np
import pytest

from harness import fitopt_cases as FC
from test_lm_core_cpu import load_lm

IDS = [c["name"] for c in FC.CASES]
WORST = dict(a=(0.0, ""), b_rel=(0.0, ""), b_abs=(0.0, ""), d=(np.inf, ""))


@pytest.fixture(scope="module")
def lm():
    return load_lm()


@pytest.fixture(autouse=True)
def _quiet():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")     # the reference's exp() overflows on the way to a pinned bound
        yield


def _note(key, value, name):
    if value > WORST[key][0]:
        WORST[key] = (value, name)


def test_table_holds_what_the_tests_need():
    opts = [c["opt"] for c in FC.CASES]
    assert {o.get("radius_fit", 5) for o in opts} == {1, 2, 3, 4, 5}
    assert {(o["min_delta_center"], o["max_delta_center"]) for o in opts if "min_delta_center" in o} >= {
        (0.25, 0.5), (2.5, 1.0), (1.5, 1.5), (4.0, 6.0)}
    assert {(o["min_w"], o["max_w"], o["init_w"]) for o in opts if "min_w" in o} >= {
        (1.0, 2.0, 1.5), (0.5, 4, 3.5), (0.2, 8.0, 0.6), (1.7, 1.9, 1.8)}
    assert {o["max_dist_th"] for o in opts if "max_dist_th" in o} >= {0.0, 1e-3, 5.0, -1.0}
    assert {o["n_max_iter"] for o in opts if o.get("max_dist_th") == 1e-3 and "n_max_iter" in o} >= {-5, -1, 0, 1, 2, 3, 5}
    assert any(c["legacy"] and c["opt"]["radius_fit"] == 4 for c in FC.CASES)
    assert any(set(o) == set(FC.DEFAULTS) and all(o[k] != FC.DEFAULTS[k] for k in o) for o in opts)
    for c in FC.CASES:     # every float32 stack also rounded to uint16
        assert any(d["field"] == c["field"] and d["dtype"] == "u16" for d in FC.CASES)
    for name, shape, least in (("iso", FC.SHAPE, 6), ("clu", FC.SHAPE, 6), ("big", FC.BIG_SHAPE, 74), ("dense", FC.BIG_SHAPE, 257)):
        im, seeds = FC.field(name)
        assert im.shape == shape and im.dtype == np.float32 and len(seeds) >= least
        assert np.array_equal(seeds, np.round(seeds))


@pytest.mark.parametrize("case", FC.CASES, ids=IDS)
def test_gate_a_host_lm_core_agrees_with_minpack(lm, case):
    a = FC.gate_a(lm, case)
    print(case["name"], "gate (a) %.3g" % a)
    _note("a", a, case["name"])
    assert a <= FC.GATE_A
    assert np.array_equal(FC.oracle(case)["nvox"] < 10, np.isnan(FC.oracle(case)["first"]).any(axis=1))


@pytest.mark.parametrize("case", [c for c in FC.CASES if c["dtype"] == "f32"],
                         ids=[c["name"] for c in FC.CASES if c["dtype"] == "f32"])
def test_gate_b_rows_are_insensitive_to_the_last_bits_of_the_input(case):
    rel, ab, same_iter = FC.gate_b(case)
    print(case["name"], "gate (b) rel %.3g abs %.3g n_iter equal %s" % (rel, ab, same_iter))
    _note("b_rel", rel, case["name"])
    _note("b_abs", ab, case["name"])
    assert rel <= FC.GATE_B_REL and ab <= FC.GATE_B_ABS and same_iter


@pytest.mark.parametrize("case", FC.CASES, ids=IDS)
def test_gate_c_no_voronoi_ties(case):
    same, ties = FC.gate_c(case)
    assert same and ties == 0


@pytest.mark.parametrize("case", FC.CASES, ids=IDS)
def test_gate_d_no_isotropic_fit(case):
    d = FC.gate_d(case)
    print(case["name"], "gate (d) %.3g" % d)
    if d < WORST["d"][0]:
        WORST["d"] = (d, case["name"])
    assert d >= FC.GATE_D


@pytest.mark.parametrize("case", FC.CASES, ids=IDS)
def test_every_option_set_bites(case):
    """the rows or n_iter differ from the same field at the defaults — by ten times the GPU bar at least, or a kernel that
    ignored the option would still pass.  (The control cases are the defaults.)"""
    o, d = FC.oracle(case), FC.oracle(FC.default_of(case))
    rel, ab = FC.row_gap(o["rows"], d["rows"])
    print(case["name"], "bite rel %.3g abs %.3g n_iter %d (defaults %d)" % (rel, ab, o["n_iter"], d["n_iter"]))
    if FC.is_control(case):
        assert rel == 0.0 and o["n_iter"] == d["n_iter"]
        return
    assert rel >= 1e-3 or o["n_iter"] != d["n_iter"]


def test_sweep_limits_truncate():
    """at max_dist_th = 1e-3 the cluster needs at least seven sweeps, so every n_max_iter of the table cuts the loop short:
    n_iter = max(n_max_iter, 0) + 1"""
    for dt in ("f32", "u16"):
        free = FC.oracle(FC.BY_NAME["dist_th_0.001-clu-%s" % dt])
        assert free["n_iter"] >= 7
        for n in (-5, -1, 0, 1, 2, 3, 5):
            assert FC.oracle(FC.BY_NAME["n_max_iter_%d-clu-%s" % (n, dt)])["n_iter"] == max(n, 0) + 1
    for n in (0, 1, 3):
        assert FC.oracle(FC.BY_NAME["sweeps_%d-big-f32" % n])["n_iter"] == n + 1
    assert FC.oracle(FC.BY_NAME["sweeps_10-big-f32"])["n_iter"] == FC.oracle(FC.BY_NAME["sweeps_10-dense-f32"])["n_iter"] == 11
    assert FC.oracle(FC.BY_NAME["sweeps_4-dense-u16"])["n_iter"] == 5


def test_bounds_are_active():
    """the width cases press spots against both bounds, the small-delta cases pin centres at theirs"""
    r = FC.oracle(FC.BY_NAME["w_1_2_1.5-mild-f32"])["rows"]
    assert (r[:, 5:8] < 1.0 + 1e-3).any() and (r[:, 5:8] > 2.0 - 1e-3).any()
    assert ((r[:, 5:8] > 1.1) & (r[:, 5:8] < 1.9)).any()
    r = FC.oracle(FC.BY_NAME["w_1.7_1.9_1.8-aniso-f32"])["rows"]
    assert (r[:, 5:8] >= 1.7 - 1e-6).all() and (r[:, 5:8] <= 1.9 + 1e-6).all()
    assert ((r[:, 5:8] < 1.7 + 1e-3).any(axis=1) & (r[:, 5:8] > 1.9 - 1e-3).any(axis=1)).all()
    case = FC.BY_NAME["delta_0.25_0.5_shifted-mild-f32"]
    r, seeds = FC.oracle(case)["rows"], FC.stack_of(case)[1]
    assert (np.abs(r[:, 1:4] - seeds).max(axis=1) > 0.5 - 1e-3).all()
    case = FC.BY_NAME["delta_2.5_1-iso-f32"]
    o, seeds = FC.oracle(case), FC.stack_of(case)[1]
    assert (np.abs(o["first"][:, 1:4] - seeds).max(axis=1) > 1.0 + 1e-3).any()     # the first fit went further than the refit may
    assert (np.abs(o["rows"][:, 1:4] - seeds).max(axis=1) <= 1.0 + 1e-6).all()


def test_gate_a_rejects_the_ill_conditioned_inputs(lm):
    """the gate can fail: two first fits on which the host LM core and MINPACK part by more than GATE_A whatever runs them"""
    import np_oracle as O
    for name, im, seeds, opt in FC.rejected_inputs():
        f = O.iter_fit_seed_points(im, seeds.T, **opt)
        f.firstfit()
        o = dict(FC.DEFAULTS, **opt)
        a = FC.gate_a_fits(lm, f.gparms, np.array(f.ps, dtype=np.float64), 0, o["min_delta_center"],
                           min_w=o["min_w"], max_w=o["max_w"], init_w=o["init_w"])
        print(name, "gate (a) %.3g" % a)
        assert a > FC.GATE_A


def test_worst_gate_values():
    """runs last: the figures of the harness's docstring"""
    print("worst gate values:", ", ".join("%s %.3g (%s)" % (k, v[0], v[1]) for k, v in WORST.items()))
    assert WORST["a"][0] <= FC.GATE_A and WORST["b_rel"][0] <= FC.GATE_B_REL and WORST["b_abs"][0] <= FC.GATE_B_ABS
    assert WORST["d"][0] >= FC.GATE_D
