"""CPU: the LM solver stopped at its evaluation (lm_advance, csrc/ia3_lm.h) against the loop lm_solve.

The fit kernel runs the two fits of a seed without neighbours through ONE driver: the evaluations one after the other,
the algebra between two evaluations for both fits at once.  That is only the parent's arithmetic if a fit driven through
lm_advance, with another fit's rounds in between, does what lm_solve does with it alone: tests/native/lm_pair_cpu.cpp
runs every fit both ways, each fit on a work area filled with junk, and the results are compared bit for bit."""
import os
import subprocess
import ctypes as C
import numpy as np
import pytest
from conftest import build_case, load_golden
import np_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "native", "liblmpaircpu.so")
N_PER_CASE = 6


@pytest.fixture(scope="module")
def lm():
    src = os.path.join(HERE, "native", "lm_pair_cpu.cpp")
    hdr = os.path.join(HERE, "..", "imageanalysis3_amd", "csrc", "ia3_lm.h")
    if not os.path.isfile(SO) or os.path.getmtime(SO) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", SO, src])
    return C.CDLL(SO)


def pair(lm, vals, X, center, delta, kind, maxfev, variant=0, iw=(0.0, 0.0, 0.0), order=0, lohi=None):
    """-> (4, 15) float64: fit 0 alone, fit 1 alone, fit 0 interleaved, fit 1 interleaved (x[10], fnorm, info, nfev,
    iter, zero diagonal entries of JtJ at the start)"""
    vals = np.ascontiguousarray(vals, dtype=np.float64)
    lohi = vals if lohi is None else np.ascontiguousarray(lohi, dtype=np.float64)
    coords = np.ascontiguousarray(np.array(X).T, dtype=np.int32)
    c = np.array(center, dtype=np.float64)
    d = np.array(delta, dtype=np.float64)
    k = np.array(kind, dtype=np.int32)
    m = np.array(maxfev, dtype=np.int32)
    w = np.array(iw, dtype=np.float64)
    out = np.full((4, 15), -777.0)
    vp = C.c_void_p
    rc = lm.ia3cpu_pair(vals.ctypes.data_as(vp), coords.ctypes.data_as(vp), C.c_int(len(vals)), lohi.ctypes.data_as(vp),
                        C.c_int(len(lohi)), c.ctypes.data_as(vp), d.ctypes.data_as(vp), k.ctypes.data_as(vp),
                        m.ctypes.data_as(vp), C.c_int(variant), w.ctypes.data_as(vp), C.c_int(order), out.ctypes.data_as(vp))
    assert rc == 0
    return out


def assert_same(out):
    """every field of both fits, bit for bit (NaN included)"""
    for f in (0, 1):
        a, b = out[f], out[2 + f]
        assert a.tobytes() == b.tobytes(), (f, a, b)


@pytest.fixture(scope="module")
def balls():
    """(case name, values, coordinates, centre, first-fit kind) of the first fits of the golden cases"""
    res = []
    for name in ("c1_f32", "c1_u16", "edge_f32", "clu_f32"):
        im = build_case(name)
        seeds = O.get_seeds(im, th_seed=600)
        f = O.iter_fit_seed_points(im, seeds.T)
        f.firstfit()
        kind = 1 if im.dtype == np.uint16 else 0
        took = 0
        for (im_, X, center) in f.gparms:
            if len(im_) < 10:
                continue
            res.append((name, np.asarray(im_, dtype=np.float64), np.asarray(X), center, kind))
            took += 1
            if took == N_PER_CASE:
                break
    assert len(res) == 4 * N_PER_CASE
    return res


@pytest.mark.parametrize("order", [0, 1])
def test_interleaved_pair_equals_two_plain_solves(lm, balls, order):
    """first fit (the stack's kind, delta 1) beside the refit (kind 2, delta 2.5) on the same voxels"""
    for name, vals, X, center, kind in balls:
        out = pair(lm, vals, X, center, (1.0, 2.5), (kind, 2), (1000, 1000), order=order)
        assert_same(out)
        assert (out[:, 11] >= 1).all() and (out[:, 11] <= 3).all(), (name, out[:, 11])   # both converge
        assert (out[:2, 12] > 3).all()


def test_start_has_two_zero_columns(lm, balls):
    """The production start point has three equal widths: the two angle columns of the Jacobian are exactly zero there,
    so the first lm_par of every such fit goes through the `skip` branch (lm_factor) — in both fits of a pair."""
    for name, vals, X, center, kind in balls:
        out = pair(lm, vals, X, center, (1.0, 2.5), (kind, 2), (1000, 1000))
        assert (out[:, 14] == 2).all(), (name, out[:, 14])
        assert_same(out)


@pytest.mark.parametrize("limited", [0, 1])
def test_one_fit_stops_at_maxfev(lm, balls, limited):
    """one fit runs out of evaluations (info 5) while the other goes on to converge: the rounds after that serve one fit"""
    for name, vals, X, center, kind in balls:
        maxfev = [1000, 1000]
        maxfev[limited] = 4
        out = pair(lm, vals, X, center, (1.0, 2.5), (kind, 2), maxfev)
        assert_same(out)
        assert out[limited, 11] == 5 and out[limited, 12] == 4, (name, out[limited])
        assert 1 <= out[1 - limited, 11] <= 3 and out[1 - limited, 12] > 4, (name, out[1 - limited])


@pytest.mark.parametrize("n", [3, 7, 9])
def test_fewer_voxels_than_parameters(lm, balls, n):
    """n < NP: JtJ has rank n at the most, pivots vanish throughout (the kernel does not fit such balls; the solver core
    must still do the same thing both ways)"""
    for name, vals, X, center, kind in balls[::3]:
        out = pair(lm, vals[:n], X[:, :n], center, (1.0, 2.5), (kind, 2), (200, 200), lohi=vals)
        assert_same(out)
        assert (out[:, 11] != 0).all()


def test_legacy_model_pair(lm):
    """FitCfg::variant 1 on the voxel sets of the legacy golden case"""
    from conftest import build_legacy
    im, m = build_legacy()
    g = load_golden("legacy.npz")
    sa = tuple(m["seeding"]["default"][:-1]) + (False,)
    iw = [np.log((16.0 - w * w) / (w * w - 0.25)) for w in (1.35, 1.9, 1.9)]
    done = 0
    for i in (0, 3):
        seeds = O.legacy_get_seed_in_distance(im, g["coords"][i], *sa)
        f = O.iter_fit_seed_points_v3(im, seeds.T, *m["fitting_args"])
        zb, xb, yb = O.ball_offsets(5)
        for ic, (zc, xc, yc) in enumerate(f.centers):
            z, x, y = O._in_dim(int(zc) + zb, int(xc) + xb, int(yc) + yb, *im.shape)
            X_full = np.array([z, x, y], dtype=int)
            X = X_full[:, f._nearest_is_me(X_full, ic)]
            vals = im[X[0], X[1], X[2]]
            for order in (0, 1):
                out = pair(lm, vals, X, (zc, xc, yc), (1.0, 2.5), (1, 2), (1100, 1100), variant=1, iw=iw, order=order)
                assert_same(out)
            done += 1
    assert done > 0
