"""Fixtures of the density clouds: tests/golden/clouds.npz.

Runs the reference's own ``visual_tools.py`` (``gauss_ker``, ``add_source``, ``subtract_source``, ``plus_source``) and
``structure_tools/chromosome.py`` (``convert_chr2Zxys_2_Cloud``, which imports ``figure_tools/plot_decode.py`` for the
centring) on the cases of tests/harness/cloud_cases.py.  ``visual_tools.py`` comes through oracle/ref_loader.py; the other
two are loaded by file, with a stand-in ``figure_tools`` package that carries the eight layout constants
``plot_decode.py`` imports.  Only outputs are stored:

    ker_<case>            gauss_ker of the case, float64
    src_<case>            add_source of the case on the 12 x 10 x 8 base image, float64
    multi_f64, multi_f32  the loop of add_source over the 70 sources of multi_case(): float64, and assigned into a float32
                          array after every source
    pfit_minus, pfit_plus subtract_source and plus_source of one 11-column fit row
    cloud_<i>_keys        the chromosomes that option set i returns, in order, joined by commas
    cloud_<i>_<chr>       their float32 clouds
    big_sum, big_samples, big_planes   the default-size cloud (100**3, one homolog of 21 loci): np.sum, the voxels of
                          cloud_cases.sample_index, and the last plane of each axis
    sig_<name>            str(inspect.signature) of the five reference functions

Needs the reference tree (IA3_REFERENCE); nothing here runs on the GPU.

    python scripts/make_cloud_golden.py

The script asserts the facts about the reference's arithmetic that csrc/ia3_cloud.h and cloud.hip are built on.
"""
import importlib.util
import inspect
import os
import sys
import types
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

OUT = os.path.join(ROOT, "tests", "golden")


def load_modules():
    import ref_loader
    _, vt = ref_loader.load_legacy()
    ft = types.ModuleType("IA3.figure_tools")
    ft.__path__ = []
    ft.__dict__.update(_dpi=300, _single_col_width=2.25, _double_col_width=4.75, _single_row_height=2, _ref_bar_length=1000,
                       _ticklabel_size=2, _ticklabel_width=0.5, _font_size=7.5)
    sys.modules["IA3.figure_tools"] = ft
    st = types.ModuleType("IA3.structure_tools")
    st.__path__ = []
    sys.modules["IA3.structure_tools"] = st

    def load(name, *path):
        spec = importlib.util.spec_from_file_location(name, os.path.join(ref_loader.REF, *path))
        m = importlib.util.module_from_spec(spec)
        sys.modules[name] = m
        spec.loader.exec_module(m)
        return m

    load("IA3.figure_tools.plot_decode", "figure_tools", "plot_decode.py")
    return vt, load("IA3.structure_tools.chromosome", "structure_tools", "chromosome.py")


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def facts(vt, ch, K):
    """Points 1 to 4 of DESIGN.md section 27, each against the reference itself."""
    # 1: the axis pairing, the division before the square, the order of the sum
    for name, (sig, s, disp) in K.ker_cases().items():
        assert same(vt.gauss_ker(sig, s, disp), K.np_gauss_ker(sig, s, disp)), name
    sig, s, disp = K.ker_cases()["ker_s7"]
    t = [K.np_axis_term(s + 1, disp[k], s, sig[k]) for k in range(3)]
    natural = np.exp(-((t[0][:, None, None] + t[1][None, :, None]) + t[2][None, None, :]) / 2.)   # axis k with entry k
    assert not np.allclose(vt.gauss_ker(sig, s, disp), natural)
    assert np.allclose(vt.gauss_ker(sig, s, disp), np.transpose(natural, (2, 0, 1)))
    z = vt.gauss_ker(*K.ker_cases()["ker_zero_sigma"])
    assert np.isnan(z[:, :, 3]).all() and (z[:, :, [0, 1, 2, 4, 5, 6]] == 0).all()
    assert np.exp(-746.0) == 0.0 and np.exp(-745.0) > 0.0 and np.exp(-np.inf) == 0.0
    # 2: truncation toward zero, the clamp that never reaches the last plane, boxes outside the image
    im = K.base_image(np.float32)
    for name, (dtype, pos, h, sig, fold) in K.source_cases().items():
        base = K.base_image(dtype)
        keep = base.copy()
        out = vt.add_source(base, pos, h, sig, fold)
        assert same(base, keep) and out.dtype == np.float64, name                # 3: a copy, in float64
        assert same(out, K.np_add_source(base, pos, h, sig, fold)), name
        assert same(out[-1], base[-1].astype(float)) and same(out[:, -1], base[:, -1].astype(float)) \
            and same(out[:, :, -1], base[:, :, -1].astype(float)), name
        if "far" in name:
            assert same(out, base.astype(float)), name
    assert not same(vt.add_source(im, (-0.5, 4.6, 3.2), 200, *K.SMALL_EVEN), im.astype(float))
    # 4: assigning the float64 result into a float32 array rounds after every source
    pos, h, sig, fold = K.multi_case()
    acc64, acc32 = im.astype(np.float64), im.copy()
    for i in range(len(pos)):
        acc64 = vt.add_source(acc64, pos[i], h[i], sig[i], fold[i])
        acc32[...] = vt.add_source(acc32, pos[i], h[i], sig[i], fold[i])
    assert same(acc64, K.np_add_sources(im, pos, h, sig, fold)) and same(acc32, K.np_add_sources(im, pos, h, sig, fold, np.float32))
    assert not same(acc32, acc64.astype(np.float32))
    return acc64, acc32


def main():
    from harness import cloud_cases as K
    warnings.simplefilter("ignore")
    vt, ch = load_modules()
    d = {}
    d["multi_f64"], d["multi_f32"] = facts(vt, ch, K)
    for name, (sig, s, disp) in K.ker_cases().items():
        d[name] = vt.gauss_ker(sig, s, disp)
    for name, (dtype, pos, h, sig, fold) in K.source_cases().items():
        d[name] = vt.add_source(K.base_image(dtype), pos, h, sig, fold)
    pfit = np.array([150.0, 5.3, 4.6, 3.2, 100.0, 0.0, 0.0, 0.0, 0.6, 0.5, 0.4])
    d["pfit_minus"] = vt.subtract_source(K.base_image(np.uint16), pfit)
    d["pfit_plus"] = vt.plus_source(K.base_image(np.uint16), pfit)
    cell = K.cell()
    for i, opt in enumerate(K.cloud_options()):
        out = ch.convert_chr2Zxys_2_Cloud(cell, **K.cloud_kwargs(opt))
        emu = K.np_cloud(cell, **K.cloud_kwargs(opt))
        assert list(out) == list(emu) and all(same(out[c], emu[c]) for c in out), opt          # 5
        d["cloud_%d_keys" % i] = np.array(",".join(out))
        for c, arr in out.items():
            assert arr.dtype == np.float32 and (arr[:, -1] == 0).all() and (arr[:, :, -1] == 0).all() and (arr[..., -1] == 0).all()
            d["cloud_%d_%s" % (i, c)] = arr
        print("option set", i, {c: len(a) for c, a in out.items()})
    big = ch.convert_chr2Zxys_2_Cloud(K.default_cell())["1"]
    assert big.shape == (1, 100, 100, 100) and same(big, K.np_cloud(K.default_cell())["1"])
    d["big_sum"] = np.sum(big)
    d["big_samples"] = big.ravel()[K.sample_index(big.size)]
    d["big_planes"] = np.stack([big[0, -1], big[0, :, -1], big[0, :, :, -1]])
    assert (d["big_planes"] == 0).all() and (d["big_samples"] > 0).any()
    for name in ("gauss_ker", "add_source", "subtract_source", "plus_source"):
        d["sig_" + name] = np.array(str(inspect.signature(getattr(vt, name))))
    d["sig_convert_chr2Zxys_2_Cloud"] = np.array(str(inspect.signature(ch.convert_chr2Zxys_2_Cloud)))
    path = os.path.join(OUT, "clouds.npz")
    np.savez_compressed(path, **d)
    print("arrays", len(d), "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
