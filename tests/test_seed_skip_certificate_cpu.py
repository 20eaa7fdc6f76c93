"""CPU: the certificate behind the plane skipping of the fused seed detector (csrc/ia3_seedskip.h, compiled with the host
compiler) against the front filter's own sequence: for every voxel, max_im by the oracle's filter is at or below the
certified bound of its unit (tile rows x 32-column strip x plane), made from the strip maxima of the axis-0 result over
the unit's window exactly as seed_front_k's prologue makes it."""
import os
import subprocess
import ctypes as C
import numpy as np
import pytest

import np_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "native", "libseedskipcpu.so")
FT_X = 16   # rows of a detector tile (seed.hip)


@pytest.fixture(scope="module")
def sk():
    src = os.path.join(HERE, "native", "seedskip_cpu.cpp")
    hdr = os.path.join(HERE, "..", "imageanalysis3_amd", "csrc", "ia3_seedskip.h")
    if not os.path.isfile(SO) or os.path.getmtime(SO) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", SO, src])
    lib = C.CDLL(SO)
    lib.skip_taps_sup.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.skip_front_bound.argtypes = [C.POINTER(C.c_float), C.c_int, C.c_double, C.c_int, C.POINTER(C.c_double)]
    lib.skip_unit_live.argtypes = [C.c_double, C.c_double, C.c_double]
    return lib


def taps_sup(sk, w7):
    w4 = (C.c_double * 4)(*[float(w7[3 + j]) for j in range(4)])
    sup = C.c_double(0.0)
    ok = sk.skip_taps_sup(w4, C.byref(sup))
    return bool(ok), sup.value


def unit_bounds(sk, in0, sup):
    """U[z, x // FT_X, y // 32] from the axis-0 result in0 (Z, X, Y), Y % 32 == 0"""
    Z, X, Y = in0.shape
    nby = Y // 32
    with np.errstate(invalid="ignore"):
        strips = np.fmax.reduce(in0.astype(np.float32).reshape(Z, X, nby, 32), axis=3)   # the column kernel: fmaxf leaves NaN out
    ntx = (X + FT_X - 1) // FT_X
    m = np.full((Z, ntx, nby), -np.inf, np.float32)
    for tx in range(ntx):
        x0 = tx * FT_X
        rows = strips[:, max(x0 - 3, 0):min(x0 + FT_X + 2, X - 1) + 1]
        for sb in range(nby):
            win = rows[:, :, max(sb - 1, 0):min(sb + 1, nby - 1) + 1]
            with np.errstate(invalid="ignore"):
                m[:, tx, sb] = np.fmax(m[:, tx, sb], np.fmax.reduce(np.fmax.reduce(win, axis=2), axis=1))
    m = np.ascontiguousarray(m)
    out = np.empty(m.size, np.float64)
    sk.skip_front_bound(m.ctypes.data_as(C.POINTER(C.c_float)), m.size, sup, int(in0.dtype == np.uint16),
                        out.ctypes.data_as(C.POINTER(C.c_double)))
    return out.reshape(m.shape), m


def check(sk, im, w7):
    ok, sup = taps_sup(sk, w7)
    assert ok
    in0 = O.correlate1d(im, w7, 0)
    with np.errstate(over="ignore", invalid="ignore"):
        max_im = O.correlate1d(O.correlate1d(in0, w7, 1), w7, 2)
    U, m = unit_bounds(sk, in0, sup)
    Z, X, Y = im.shape
    Uv = np.repeat(np.repeat(U, FT_X, axis=1)[:, :X], 32, axis=2)
    with np.errstate(invalid="ignore"):
        bad = max_im.astype(np.float64) > Uv          # a NaN max_im is never a candidate: not counted
    assert not bad.any(), (im.dtype, int(bad.sum()), max_im[bad][:4], Uv[bad][:4])
    return U, m


SIGMAS = (0.63, 0.75, 0.87)   # radius int(4 * sigma + 0.5) = 3


def gtaps(sigma):
    w, r = O.gaussian_kernel1d(sigma, 4.0)
    assert r == 3
    return w


@pytest.mark.parametrize("sigma", SIGMAS)
def test_random_stacks(sk, sigma):
    rng = np.random.default_rng(11)
    w = gtaps(sigma)
    f = rng.gamma(2.0, 150.0, size=(7, 41, 96)).astype(np.float32)
    f[3, 20, 40] = 9000.0
    U, m = check(sk, f, w)
    assert np.isfinite(U).all() and (U <= m * (1 + 1e-6)).all()      # the bound is a claim, not +inf
    u = rng.integers(0, 3000, size=(7, 41, 96)).astype(np.uint16)
    u[2, 0, 95] = 60000
    U, m = check(sk, u, w)
    assert np.isfinite(U).all() and (U <= m + 1).all()


@pytest.mark.parametrize("sigma", SIGMAS)
def test_constant_stacks(sk, sigma):
    """on a constant stack the filter returns (nearly) the constant: the taps' sum and its rounding are what matter"""
    w = gtaps(sigma)
    for c in (1000.0, 0.1, 1.0 / 3.0, 16777217.0, 3.0e-39, 0.0):
        U, m = check(sk, np.full((5, 20, 64), c, np.float32), w)
        assert (U <= m * (1 + 1e-6)).all()
    for c in (777, 1, 0, 65535):
        U, m = check(sk, np.full((5, 20, 64), c, np.uint16), w)
        assert (U <= m + 1).all()


def test_top_of_range(sk):
    w = gtaps(0.75)
    rng = np.random.default_rng(12)
    u = rng.integers(65000, 65536, size=(5, 33, 64)).astype(np.uint16)
    u[1, 5, 5] = 65535
    check(sk, u, w)
    big = (rng.random((5, 33, 64)) * 3.0e38).astype(np.float32)     # sums overflow to +inf: the unit is live
    check(sk, big, w)
    check(sk, (rng.random((5, 33, 64)) * 1.0e30).astype(np.float32), w)


def test_negative_and_mixed_sign(sk):
    w = gtaps(0.75)
    rng = np.random.default_rng(13)
    neg = (-rng.gamma(2.0, 50.0, size=(6, 30, 96)) - 1.0).astype(np.float32)
    U, m = check(sk, neg, w)
    assert np.isinf(U).all()                                        # a negative maximum makes no claim
    mixed = rng.normal(0, 50, size=(6, 30, 96)).astype(np.float32)
    mixed[2, 10, 50] = 900.0
    mixed[4, 20, 70] = -4000.0
    check(sk, mixed, w)
    mixed[:, :, :32] = -np.abs(mixed[:, :, :32]) - 1.0              # strips whose maximum is negative beside positive ones
    check(sk, mixed, w)


def test_nan_and_inf(sk):
    w = gtaps(0.75)
    rng = np.random.default_rng(14)
    f = rng.gamma(2.0, 150.0, size=(6, 30, 96)).astype(np.float32)
    f[3, 10, 40] = np.nan
    f[2, 20, 70] = np.inf
    U, m = check(sk, f, w)
    assert np.isinf(U[1:4, 1, 2]).all()                             # +inf in the window: live


def test_explicit_taps_and_refusals(sk):
    rng = np.random.default_rng(15)
    f = rng.gamma(2.0, 150.0, size=(5, 30, 64)).astype(np.float32)
    check(sk, f, np.full(7, 1.0 / 7.0))
    check(sk, f, np.full(7, 0.2))                                   # taps' sum 1.4
    check(sk, f, np.array([0.0, 0.0, 0.25, 0.5, 0.25, 0.0, 0.0]))
    ok, _ = taps_sup(sk, np.array([0.01, -0.05, 0.3, 0.48, 0.3, -0.05, 0.01]))
    assert not ok                                                   # a negative tap is refused
    ok, _ = taps_sup(sk, np.array([0.0, 0.1, 0.2, np.nan, 0.2, 0.1, 0.0]))
    assert not ok
    ok, _ = taps_sup(sk, np.zeros(7))
    assert not ok
    ok, _ = taps_sup(sk, np.full(7, 1e300))
    assert not ok


def test_unit_live_matches_the_detectors_test(sk):
    """live <=> U - bound >= th_test, the detector's own expression; NaN / +inf bounds fail, -inf passes"""
    assert sk.skip_unit_live(700.0, 90.0, 600.0) == 1
    assert sk.skip_unit_live(689.0, 90.0, 600.0) == 0
    assert sk.skip_unit_live(np.inf, 90.0, 600.0) == 1
    assert sk.skip_unit_live(np.inf, np.inf, 600.0) == 0
    assert sk.skip_unit_live(700.0, np.nan, 600.0) == 0
    assert sk.skip_unit_live(0.0, -np.inf, 600.0) == 1
