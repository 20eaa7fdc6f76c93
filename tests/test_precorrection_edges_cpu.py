"""CPU: the inputs of the pre-correction edge tests discriminate, and np_oracle is the reference on them.

tests/golden/precorr_edges.json holds what the reference's own functions returned on the inputs of
tests/harness/precorr_ref.py (scripts/make_precorr_edge_golden.py); here np_oracle reproduces every one of them, and the
rule statements of the harness (the uint16 cast, the sequential channel sum) are pinned to NumPy.  The counts asserted
below are conditions on the inputs: without them a kernel could pass tests/test_gpu_precorrection_edges.py while being
wrong in the branch the input was meant to reach."""
import json
import os

import numpy as np
import pytest
from conftest import GOLDEN
from harness import precorr_ref as P
import np_oracle as O


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "precorr_edges.json")) as f:
        return json.load(f)


def test_golden_lists_exactly_the_cases(golden):
    assert sorted(golden["crc"]) == sorted(P.CASES)
    # the only cases the reference could not be driven on: a float64 mix through correct_fov_image (it casts to float32)
    assert sorted(golden["sources"]) == sorted(k for k in P.keys("bleed") if k.endswith("/f64"))


@pytest.mark.parametrize("kind", ["illum", "bleed", "illum_rescale", "bleed_rescale", "hot", "zshift"])
def test_oracle_reproduces_the_reference(golden, kind):
    bad = [k for k in P.keys(kind) if [P.crc(o) for o in P.oracle(k)] != golden["crc"][k]]
    assert not bad, bad


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_numpy_cast_is_the_documented_rule(dtype):
    v = np.array(P.CAST_EDGES, dtype=dtype)
    want = P.to_u16(v)
    assert list(want[:6]) == [70000 - 65536, 65535, 65535, 0, 65535, 0] and not want[7:14].any() and want[14] == 0
    assert want[6] == (2147483520 & 0xFFFF)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(v.astype(np.uint16), want)
        wide = np.zeros((len(v), 3), dtype)
        wide[:, 1] = v
        assert np.array_equal(wide[:, 1].astype(np.uint16), want)               # strided source
        assert np.array_equal(np.tile(v, 37).astype(np.uint16), np.tile(want, 37))   # long enough for the SIMD loops
        assert np.array_equal(np.tile(v, 37)[::3].astype(np.uint16), np.tile(want, 37)[::3])


@pytest.mark.parametrize("dt", list(P.DTYPES))
@pytest.mark.parametrize("C", [1, 2, 3, 4, 8])
def test_sequential_mix_is_numpys(C, dt):
    key = "bleed/C%d/3x17x19/%s" % (C, dt)
    ims, pf = P.inputs(key)
    assert pf.dtype == P.DTYPES[dt] and np.isnan(pf).sum() == 1 and np.isposinf(pf).sum() == 1 and np.isneginf(pf).sum() == 1
    seq = P.bleed_sequential(ims, pf)
    for a in range(C):
        assert P.n_diff(seq[a], P.oracle(key)[a]) == 0, (a, P.n_diff(seq[a], P.oracle(key)[a]))
    if C == 8 and dt == "f32":   # the order of the sum is visible in the result
        rev = P.bleed_sequential(ims, pf, order=range(C - 1, -1, -1))
        assert sum(P.n_diff(rev[a], seq[a]) for a in range(C)) >= 1


@pytest.mark.parametrize("arith", ["u16", "f32"])
@pytest.mark.parametrize("name", P.RANDOM_HOT)
def test_random_hot_fields_depend_on_candidate_order(name, arith):
    im, hot_pix_th, hot_th = P.inputs("hot/%s/%s" % (name, arith))
    xs, ys = P.hot_candidates(im, hot_pix_th, hot_th)
    fwd = P.hot_replace(im, xs, ys).astype(np.uint16)
    assert P.n_diff(fwd, P.oracle("hot/%s/%s" % (name, arith))[0]) == 0
    assert P.n_diff(P.hot_replace(im, xs[::-1], ys[::-1]).astype(np.uint16), fwd) > 0


def test_hot_pixel_counts(golden):
    for key in P.keys("hot"):
        im, hot_pix_th, hot_th = P.inputs(key)
        xs, ys = P.hot_candidates(im, hot_pix_th, hot_th)
        n_in = int(P.interior(xs, ys, im.shape).sum())
        assert golden["counts"][key] == dict(n_hot=len(xs), n_interior=n_in), key
        name = P.CASES[key][1]
        if name == "lattice0":
            assert (len(xs), n_in) == (P.HOT_CAP, P.HOT_CAP)        # the last count the device list holds
        elif name == "lattice1":
            assert (len(xs), n_in) == (P.HOT_CAP + 1, P.HOT_CAP + 1)
        elif name == "rand_big":
            assert n_in > P.HOT_CAP                                  # host fallback in both arithmetics
        elif name == "border":
            assert len(xs) == 4 and n_in == 0
            assert sorted(zip(xs.tolist(), ys.tolist())) == [(0, 3), (2, 0), (6, 10), (8, 5)]
        elif name == "single":
            assert (xs.tolist(), ys.tolist()) == ([1], [1])
        else:
            assert 1000 < n_in <= P.HOT_CAP                          # device list


@pytest.mark.parametrize("arith", ["u16", "f32"])
def test_large_hot_field_has_borders_neighbours_and_wraps(arith, golden):
    im, hot_pix_th, hot_th = P.inputs("hot/rand_big/%s" % arith)
    Z, X, Y = im.shape
    assert X % 4 != 0 and Y % 64 != 0                                # partial tiles of the vote kernel
    xs, ys = P.hot_candidates(im, hot_pix_th, hot_th)
    assert (xs == 0).any() and (xs == X - 1).any() and (ys == 0).any() and (ys == Y - 1).any()
    m = np.zeros((X, Y), bool)
    m[xs, ys] = True
    assert int((m[:, 1:] & m[:, :-1]).sum() + (m[1:] & m[:-1]).sum()) >= 100
    if arith == "u16":
        wraps = P.wrapping_sums(im)                                  # uint16 neighbour sums that wrap, per plane
        assert wraps == golden["counts"]["hot/rand_big/wrapping_sums"] == [9636, 9637, 9637], wraps   # 8 % of a plane


def test_edge_profile_reaches_every_class_of_the_cast(golden):
    im, p32 = P.inputs("illum/4x17x19/f32")
    _, p64 = P.inputs("illum/4x17x19/f64")
    assert p32.dtype == np.float32 and p64.dtype == np.float64
    with np.errstate(all="ignore"):
        for key, pf in (("illum/4x17x19/f32", p32), ("illum/4x17x19/f64", p64)):
            q = im.astype(np.float32) / pf[None]
            n = P.quotient_census(q)
            assert n == golden["counts"][key]
            assert n["wrap"] >= 100 and n["overflow"] >= 4 and n["negative"] >= 4 and n["nan"] >= 1, n
            assert P.n_diff(P.to_u16(q), P.oracle(key)[0]) == 0
            assert P.n_diff(P.saturating_u16(q), P.oracle(key)[0]) > 0
    assert P.n_diff(P.oracle("illum/4x17x19/f32")[0], P.oracle("illum/4x17x19/f64")[0]) > 0
    for shape in P.ILLUM_SHAPES:   # four-wide kernel only where the plane is a multiple of four
        assert (shape[1] * shape[2] % 4 == 0) == (shape in ((4, 16, 20), (2, 2, 2)))


@pytest.mark.parametrize("dt", list(P.DTYPES))
def test_rescale_of_a_nan_or_inf_quotient_is_all_zero(dt):
    for kind in ("nan", "inf"):
        im, pf, _ = P.inputs("illum_rescale/%s/3x17x19/%s/r1" % (kind, dt))
        with np.errstate(all="ignore"):
            q = im.astype(np.float32) / pf[None]
            assert (np.isnan(q).any(), np.isinf(q).any()) == ((True, False) if kind == "nan" else (False, True))
            assert not O.daxp_illumination(im, pf, rescale=True).any()
        assert not P.oracle("illum_rescale/%s/3x17x19/%s/r1" % (kind, dt))[0].any()
        assert P.oracle("illum_rescale/%s/3x17x19/%s/r0" % (kind, dt))[0].any()
    assert P.oracle("illum_rescale/ordinary/3x17x19/%s/r1" % dt)[0].max() == 65535


def _tree_min(vals, propagate):
    """Slot 0 of the kernels' shared-memory tree over ``vals`` (a power of two of them); ``propagate`` False is the plain
    `a < b ? a : b`, which drops a NaN candidate."""
    s, k = list(vals), len(vals) // 2
    while k:
        for t in range(k):
            a, b = s[t + k], s[t]
            s[t] = a if (a < b or (propagate and a != a)) else b
        k //= 2
    return s[0]


def _staged_min(q, thread=True, block=True, final=True):
    """The minimum of the flat quotients ``q`` through the kernels' three stages (thread loop, block tree, tree over the
    block partials), each with or without NaN propagation.  Blocks that see no voxel keep +inf."""
    B = P.MINMAX_BLOCK
    assert q.size <= 1024 * B                         # one voxel per thread at most
    part = []
    for b in range(-(-q.size // B)):
        vals = [np.inf] * B
        for t, v in enumerate(q[b * B:(b + 1) * B]):
            vals[t] = v if (v < np.inf or (thread and v != v)) else np.inf
        part.append(_tree_min(vals, block))
    return part, _tree_min(part + [np.inf] * (1024 - len(part)), final)


@pytest.mark.parametrize("dt", list(P.DTYPES))
@pytest.mark.parametrize("shape", P.RESCALE_SHAPES)
def test_far_nan_column_needs_every_reduction_level(shape, dt):
    """Only the "nan_far" inputs tell whether the second reduction level propagates NaN: every NaN voxel sits in a block
    after the first, so the first partial (the running value of the last tree) is finite."""
    tag = "x".join(str(v) for v in shape)
    B = P.MINMAX_BLOCK
    assert all(v >= B for v in P.nan_voxels("nan_far", shape)) and min(P.nan_voxels("nan", shape)) < B
    assert len({v // B for v in P.nan_voxels("nan_far", shape)}) == shape[0]         # one later block per plane
    for kind in ("nan", "nan_far"):
        im, pf, _ = P.inputs("illum_rescale/%s/%s/%s/r1" % (kind, tag, dt))
        with np.errstate(all="ignore"):
            q = (im.astype(np.float32) / pf[None]).reshape(-1)
        assert np.flatnonzero(np.isnan(q)).tolist() == P.nan_voxels(kind, shape) and not np.isinf(q).any()
        part, mn = _staged_min(q)
        assert np.isnan(mn) and np.isnan(part[0]) == (kind == "nan")
        assert not np.isnan(_staged_min(q, thread=False)[1]) and not np.isnan(_staged_min(q, block=False)[1])
        # without propagation in the last tree the near column still ends NaN; the far one does not
        assert np.isnan(_staged_min(q, final=False)[1]) == (kind == "nan")
        assert not P.oracle("illum_rescale/%s/%s/%s/r1" % (kind, tag, dt))[0].any()
        for C in (2, 3):
            ims, mix, _ = P.inputs("bleed_rescale/%s/C%d/%s/%s/r1" % (kind, C, tag, dt))
            with np.errstate(all="ignore"):
                acc = sum(ims[j].astype(mix.dtype) * mix[C - 1, j] for j in range(C)).reshape(-1)
            assert np.flatnonzero(np.isnan(acc)).tolist() == P.nan_voxels(kind, shape)


def test_rescaled_mix_inputs():
    for dt in P.DTYPES:
        for C in (2, 3):
            for kind in ("nan", "nan_far"):
                o = P.oracle("bleed_rescale/%s/C%d/3x17x19/%s/r1" % (kind, C, dt))
                assert not o[C - 1].any() and all(o[a].any() for a in range(C - 1))     # NaN reaches one output only
            o = P.oracle("bleed_rescale/inf/C%d/3x17x19/%s/r1" % (C, dt))
            assert not o[0].any() and all(o[a].any() for a in range(1, C))
            assert not any(a.any() for a in P.oracle("bleed_rescale/constant/C%d/3x17x19/%s/r1" % (C, dt)))
            assert all(a.any() for a in P.oracle("bleed_rescale/constant/C%d/3x17x19/%s/r0" % (C, dt)))


def test_z_shift_inputs():
    for name in ("z65", "z130"):
        Z = P.inputs("zshift/" + name)[0].shape[0]
        assert 2 * (Z + 1) > 64 and Z + 1 > 64                       # second blocks of sel_pick_k / sel_median_k
    f = P.inputs("zshift/f32neg")[0]
    assert f.dtype == np.float32 and (f < 0).sum() > 50 and (np.median(f, axis=(1, 2)) < 0).any()
    with np.errstate(all="ignore"):
        q = f / np.median(f, axis=(1, 2))[:, None, None] * np.median(f)
        assert ((q >= 65536) | (q < 0)).sum() > 20                   # outputs that wrap
    z = P.inputs("zshift/zero_plane")[0]
    assert np.median(z[2]) == 0 and z[2].any() and not P.oracle("zshift/zero_plane")[0][2].any()
    c = P.inputs("zshift/const_planes")[0]
    assert all(len(np.unique(pl)) == 1 for pl in c) and len(np.unique(c)) == len(c)
    assert P.inputs("zshift/tiny")[0].shape == (3, 1, 2)
