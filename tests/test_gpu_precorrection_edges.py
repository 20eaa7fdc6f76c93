"""GPU: the elementwise pre-corrections (csrc/corrections.hip, csrc/hotpix.hip) at their untested branches and cast
edges, bit for bit against np_oracle on the inputs of tests/harness/precorr_ref.py (pinned to the reference by
tests/test_precorrection_edges_cpu.py and tests/golden/precorr_edges.json).

  illumination   illum_k (planes of 17 x 19 and 1 x 5) and illum4_k (16 x 20, 2 x 2), float32 and float64 profiles,
                 host entry and resident entry out of place and in place; profile entries that make every class of
                 the final cast: wrapping, beyond int32, negative, inf, NaN
  bleedthrough   bleed_k for C = 1, 2, 3, 4, 8 on an odd plane and C = 4 on an aligned one, bleed3x4_k for C = 3 on
                 the aligned plane; NaN and +-inf in the mix; refused calls (nine channels, aliased output)
  rescale        illum_minmax_k / bleed_minmax_k / minmax_final_k with NaN and inf among the values, max == min, and a
                 stack smaller than one block; the NaN column once in the first block of the reduction and once
                 ("nan_far") only in later ones, where the tree over the block partials has to carry it
  hot pixels     hot_vote_k / hot_vote_u16f_k on partial tiles, hot_compact_k's device list up to its last entry and
                 the host fallback one candidate later, hot_fix_k / hot_fix_u16f_k over thousands of candidates whose
                 order matters
  z shift        second blocks of sel_pick_k / sel_median_k, negative float32 keys, a median of 0, ties

The pointer-alignment fallbacks of launch_illum / launch_bleed are not reached: every allocation is aligned.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
from conftest import GOLDEN
from harness import precorr_ref as P
from harness import replay as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "precorr_edges.json")) as f:
        return json.load(f)


def same(got, ref, what):
    d = P.n_diff(got, ref)
    assert d == 0, "%s: %d of %d voxels differ" % (what, d, ref.size)


def _L():
    from imageanalysis3_amd import _lib as L
    return L


def _buffer(pf):
    from imageanalysis3_amd.io_tools.load import DeviceBuffer
    return DeviceBuffer(pf)


# ---- illumination ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", P.keys("illum"))
def test_illumination_edges(key):
    from imageanalysis3_amd.io_tools.load import illumination_correction
    L = _L()
    im, pf = P.inputs(key)
    ref = P.oracle(key)[0]
    same(illumination_correction(im, pf), ref, key + " host entry")
    buf = _buffer(pf)
    try:
        with L.DeviceStack.upload(im) as s, L.DeviceStack.empty(im.shape, np.uint16) as out:
            L.check(L.lib().ia3_illumination_correct_dev(s._h, buf.ptr, buf.dtype_code, out._h))
            same(out.download(), ref, key + " resident")
            same(s.download(), im, key + " resident: input untouched")
            L.check(L.lib().ia3_illumination_correct_dev(s._h, buf.ptr, buf.dtype_code, s._h))
            same(s.download(), ref, key + " resident, in place")
    finally:
        buf.free()


# ---- bleedthrough ----------------------------------------------------------------------------------------------

def _mix_resident(ims, pf, outs_alias=None):
    """ia3_bleedthrough_correct_dev on uploaded stacks; ``outs_alias``: index of the input that output 0 aliases."""
    L = _L()
    n = len(ims)
    buf = _buffer(pf)
    ins = [L.DeviceStack.upload(im) for im in ims]
    outs = [L.DeviceStack.empty(ims[0].shape, np.uint16) for _ in ims]
    try:
        oh = [o._h for o in outs]
        if outs_alias is not None:
            oh[0] = ins[outs_alias]._h
        a_in = (C.c_void_p * n)(*[s._h for s in ins])
        a_out = (C.c_void_p * n)(*oh)
        L.check(L.lib().ia3_bleedthrough_correct_dev(a_in, n, buf.ptr, buf.dtype_code, a_out))
        return [o.download() for o in outs]
    finally:
        for s in ins + outs:
            s.free()
        buf.free()


@pytest.mark.parametrize("key", P.keys("bleed"))
def test_bleedthrough_edges(key):
    from imageanalysis3_amd.io_tools.load import bleedthrough_correction
    ims, pf = P.inputs(key)
    ref = P.oracle(key)
    for entry, got in (("host entry", bleedthrough_correction(ims, pf)), ("resident", _mix_resident(ims, pf))):
        assert len(got) == len(ref)
        for a in range(len(ref)):
            same(got[a], ref[a], "%s %s, output %d" % (key, entry, a))


def test_bleedthrough_refusals_leave_the_library_usable():
    from imageanalysis3_amd.io_tools.load import bleedthrough_correction
    rng = np.random.RandomState(0)
    nine = [rng.randint(0, 65536, size=(1, 2, 2)).astype(np.uint16) for _ in range(9)]
    pf9 = np.ones((9, 9, 2, 2), np.float32)
    with pytest.raises(NotImplementedError, match="channels supported"):
        bleedthrough_correction(nine, pf9)
    with pytest.raises(NotImplementedError, match="channels supported"):
        _mix_resident(nine, pf9)
    key = "bleed/C3/3x16x20/f32"
    ims, pf = P.inputs(key)
    with pytest.raises(ValueError, match="alias"):
        _mix_resident(ims, pf, outs_alias=2)
    for a, got in enumerate(_mix_resident(ims, pf)):
        same(got, P.oracle(key)[a], "%s after the refused calls, output %d" % (key, a))
    for a, got in enumerate(bleedthrough_correction(ims, pf)):
        same(got, P.oracle(key)[a], "%s host entry after the refused calls, output %d" % (key, a))


# ---- rescale variants ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", P.keys("illum_rescale"))
def test_illumination_rescale_edges(key):
    L = _L()
    im, pf, rescale = P.inputs(key)
    ref = P.oracle(key)[0]
    st = {"a": L.DeviceStack.upload(im)}
    try:
        R.illumination_rescaled(st, ["a"], {"a": pf}, rescale)
        same(st["a"].download(), ref, key)
    finally:
        R.free_all(st)
    buf = _buffer(pf)
    try:
        with L.DeviceStack.upload(im) as s:   # in place: `out` is the input stack
            L.check(L.lib().ia3_illumination_rescale_dev(s._h, buf.ptr, buf.dtype_code, int(rescale), s._h))
            same(s.download(), ref, key + " in place")
    finally:
        buf.free()


@pytest.mark.parametrize("key", P.keys("bleed_rescale"))
def test_bleedthrough_rescale_edges(key):
    L = _L()
    ims, pf, rescale = P.inputs(key)
    ref = P.oracle(key)
    chs = [str(j) for j in range(len(ims))]
    st = {c: L.DeviceStack.upload(im) for c, im in zip(chs, ims)}
    try:
        R.bleedthrough_rescaled(st, chs, pf, rescale)
        for a, c in enumerate(chs):
            same(st[c].download(), ref[a], "%s, output %d" % (key, a))
    finally:
        R.free_all(st)


# ---- hot pixels ------------------------------------------------------------------------------------------------

def _hot_resident(im, hot_pix_th, hot_th, float_arith):
    L = _L()
    n = C.c_int(-1)
    with L.DeviceStack.upload(im) as s:
        L.check(L.lib().ia3_remove_hot_pixels_dev(s._h, C.c_double(hot_pix_th), C.c_double(hot_th), int(float_arith),
                                                  C.byref(n)))
        return s.download(), n.value


@pytest.mark.parametrize("name", list(P.HOT_FIELDS))
def test_hot_pixels_in_image_dtype(name, golden):
    """uint16 votes and means (sums wrap): hot_vote_k<uint16_t>, hot_fix_k<uint16_t>."""
    from imageanalysis3_amd.correction_tools.filter import Remove_Hot_Pixels
    key = "hot/%s/u16" % name
    im, hot_pix_th, hot_th = P.inputs(key)
    ref = P.oracle(key)[0]
    out = Remove_Hot_Pixels(im, np.uint16, hot_pix_th=hot_pix_th, hot_th=hot_th)
    assert out is not im and out.dtype == np.uint16
    same(out, ref, key + " shim")
    got, n_hot = _hot_resident(im, hot_pix_th, hot_th, 0)
    assert n_hot == golden["counts"][key]["n_hot"]
    same(got, ref, key + " resident")
    if name == "border":
        same(out, im, key + ": nothing replaced")


@pytest.mark.parametrize("name", list(P.HOT_FIELDS))
def test_hot_pixels_float32_stack(name, golden):
    """A float32 stack, as the reference's chain passes: hot_vote_k<float>, hot_fix_k<float>, one cast at the end."""
    from imageanalysis3_amd.correction_tools.filter import Remove_Hot_Pixels
    key = "hot/%s/f32" % name
    im, hot_pix_th, hot_th = P.inputs(key)
    assert im.dtype == np.float32
    ref = P.oracle(key)[0]
    out = Remove_Hot_Pixels(im, dtype=np.uint16, hot_pix_th=hot_pix_th, hot_th=hot_th)
    assert out is not im and out.dtype == np.uint16
    same(out, ref, key + " shim")
    got, n_hot = _hot_resident(im, hot_pix_th, hot_th, 0)
    assert n_hot == golden["counts"][key]["n_hot"] and got.dtype == np.float32
    same(got.astype(np.uint16), ref, key + " resident")


@pytest.mark.parametrize("name", list(P.HOT_FIELDS))
def test_hot_pixels_uint16_storage_float32_arithmetic(name, golden):
    """The resident chain's form: hot_vote_u16f_k, hot_mark_k, hot_fix_u16f_k.  Its reference is the float32 result cast
    once at the end."""
    key = "hot/%s/f32" % name
    im, hot_pix_th, hot_th = P.inputs("hot/%s/u16" % name)
    got, n_hot = _hot_resident(im, hot_pix_th, hot_th, 1)
    assert n_hot == golden["counts"][key]["n_hot"]
    same(got, P.oracle(key)[0], key + " in uint16 storage")


# ---- z shift ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(P.ZSHIFT))
def test_z_shift_edges(name):
    from imageanalysis3_amd.corrections import Z_Shift_Correction
    L = _L()
    key = "zshift/" + name
    im, = P.inputs(key)
    ref = P.oracle(key)[0]
    same(Z_Shift_Correction(im), ref, key + " host entry")
    with L.DeviceStack.upload(im) as s:
        if im.dtype == np.uint16:   # as the chain calls it: in place
            L.check(L.lib().ia3_z_shift_correction_dev(s._h, s._h))
            same(s.download(), ref, key + " resident, in place")
        else:
            with L.DeviceStack.empty(im.shape, np.uint16) as out:
                L.check(L.lib().ia3_z_shift_correction_dev(s._h, out._h))
                same(out.download(), ref, key + " resident")
