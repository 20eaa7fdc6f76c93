"""CPU: the host-compilable arithmetic of the radix select (csrc/ia3_order.h, built by tests/native/select_cpu.cpp)
against NumPy: the key maps, a host select made of the same "pick the bin" and regroup steps, the median rules and the
percentile rule."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from harness import illum_ref

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "native", "libselectcpu.so")
DTYPES = (("u16", np.uint16), ("f32", np.float32), ("f64", np.float64))


@pytest.fixture(scope="module")
def native():
    src = os.path.join(HERE, "native", "select_cpu.cpp")
    dep = os.path.join(HERE, "..", "imageanalysis3_amd", "csrc", "ia3_order.h")
    if not os.path.isfile(SO) or os.path.getmtime(SO) < max(os.path.getmtime(src), os.path.getmtime(dep)):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", SO, src])
    lib = C.CDLL(SO)
    lib.sel_median_f32.restype = C.c_float
    lib.sel_median_u16_f32.restype = C.c_float
    for name in ("sel_median_f64", "sel_median_u16", "sel_percentile"):
        getattr(lib, name).restype = C.c_double
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _special(dt):
    """Values in ascending order (the two zeros tie), then NaNs of both signs."""
    if dt == np.uint16:
        return np.array([0, 1, 2, 255, 256, 257, 32767, 32768, 65534, 65535], dt), 0
    fi = np.finfo(dt)
    tiny = np.nextafter(dt(0), dt(1))                       # the smallest denormal
    pos = [tiny, 2 * tiny, fi.tiny / 2, fi.tiny, dt(1) - fi.epsneg, dt(1), dt(1) + fi.eps, dt(255.5), fi.max / 2, fi.max, np.inf]
    vals = np.array([-v for v in reversed(pos)] + [-0.0, 0.0] + pos, dt)
    bits = np.uint32 if dt == np.float32 else np.uint64
    nan = np.array([np.nan], dt)
    neg_nan = (nan.view(bits) | bits(1 << (8 * nan.itemsize - 1))).view(dt)
    payload = (nan.view(bits) | bits(5)).view(dt)
    return np.concatenate([vals, nan, neg_nan, payload]), 3


@pytest.mark.parametrize("name,dt", DTYPES)
def test_keys_are_monotone_and_invertible(native, name, dt):
    v, n_nan = _special(dt)
    keys = np.empty(len(v), np.uint64)
    back = np.empty(len(v), dt)
    getattr(native, "sel_keys_" + name)(_p(v), len(v), _p(keys), _p(back))
    real = len(v) - n_nan
    assert back[:real].tobytes() == v[:real].tobytes()                      # -0 and +0 come back as themselves
    assert np.all(np.diff(keys[:real].astype(object)) > 0)                  # strictly: -0 before +0
    bits = np.dtype(dt).itemsize * 8
    if n_nan:
        assert np.all(keys[real:] == np.uint64(2 ** bits - 1)) and keys[real - 1] < keys[real]
        assert np.all(np.isnan(back[real:]))
    assert int(keys.max()) < 2 ** bits
    # the order of the keys is the order of np.sort on a shuffled copy
    perm = np.random.default_rng(3).permutation(len(v))
    assert np.array_equal(np.sort(v[perm]), v[perm][np.argsort(keys[perm], kind="stable")], equal_nan=True)


def _arrays(dt, n, rng):
    """Arrays of n values: spread over the whole key range, tightly tied, and (floats) with zeros, infinities and NaNs."""
    if dt == np.uint16:
        return [rng.integers(0, 65536, n).astype(dt), rng.integers(300, 304, n).astype(dt),
                np.where(rng.random(n) < 0.5, rng.integers(0, 256, n), rng.integers(65280, 65536, n)).astype(dt)]
    wide = (rng.standard_normal(n) * 10.0 ** rng.integers(-40 if dt == np.float32 else -310, 30, n)).astype(dt)
    tied = rng.integers(-2, 3, n).astype(dt)
    special = rng.choice(np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0], dt), n)
    return [wide, tied, np.where(rng.random(n) < 0.3, special, wide), special]


@pytest.mark.parametrize("name,dt", DTYPES)
@pytest.mark.parametrize("n", [1, 2, 35, 1000])
def test_host_select_equals_sorted_at_every_rank(native, name, dt, n):
    rng = np.random.default_rng(100 + n)
    fn = getattr(native, "sel_select_" + name)
    for a in _arrays(dt, n, rng):
        want = np.sort(a)
        got = np.empty(n, dt)
        for first in range(0, n, 16):
            ranks = np.arange(first, min(first + 16, n), dtype=np.uint64)
            out = np.empty(len(ranks), dt)
            ngrp = fn(_p(a), C.c_size_t(n), _p(ranks), len(ranks), _p(out))
            keys = np.empty(len(ranks), np.uint64)
            getattr(native, "sel_keys_" + name)(_p(out), len(ranks), _p(keys), _p(np.empty(len(ranks), dt)))
            assert ngrp == len(np.unique(keys))                      # one group per distinct key at the end
            got[first:first + len(ranks)] = out
        # values with == (so -0 and +0 tie, as they do for np.sort), NaN where NaN is the answer
        assert np.array_equal(got, want, equal_nan=True)
    # repeated and unordered ranks
    a = _arrays(dt, n, rng)[0]
    ranks = np.array([n - 1, 0, n // 2, n // 2, 0, (n - 1) // 2], np.uint64)
    out = np.empty(len(ranks), dt)
    fn(_p(a), C.c_size_t(n), _p(ranks), len(ranks), _p(out))
    assert np.array_equal(out, np.sort(a)[ranks.astype(np.int64)])


@pytest.mark.parametrize("n", [1, 2, 3, 34, 35])
def test_median_rules_equal_np_median(native, n):
    rng = np.random.default_rng(n)
    for scale in (1.0, 3e38):                 # near FLT_MAX: an odd count returns the value, an even one overflows as NumPy does
        f = np.sort((rng.random(n) * scale).astype(np.float32))
        with np.errstate(over="ignore"):
            want = np.median(f)
        got = np.float32(native.sel_median_f32(_p(f), C.c_size_t(n)))
        assert want.dtype == np.float32 and got.tobytes() == want.tobytes(), (n, scale)
    d = np.sort(rng.standard_normal(n) * 1e300)
    with np.errstate(over="ignore"):
        assert np.float64(native.sel_median_f64(_p(d), C.c_size_t(n))).tobytes() == np.median(d).tobytes()
    u = np.sort(rng.integers(0, 65536, n).astype(np.uint16))
    assert native.sel_median_u16(_p(u), C.c_size_t(n)) == np.median(u)
    # the z-shift takes the median of the stack as float32
    assert np.float32(native.sel_median_u16_f32(_p(u), C.c_size_t(n))) == np.median(u.astype(np.float32))


def test_percentile_rule_equals_the_restatement(native):
    rng = np.random.default_rng(11)
    for n in (1, 2, 7, 1000):
        a = np.sort(rng.integers(0, 65536, n).astype(np.float64))
        for per in (0, 0.25, 5, 33.3, 50, 90, 99.5, 99.9, 100):
            got = native.sel_percentile(_p(a), C.c_longlong(n), C.c_double(per))
            assert got == illum_ref.score_at_percentile(a, per), (n, per)
