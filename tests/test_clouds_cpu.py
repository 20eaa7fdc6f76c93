"""No GPU: the reference's names and signatures of the Gaussian sources (visual_tools.py) and of
structure_tools/chromosome.py, the argument errors that come before any device call, the NumPy restatement of the
reference's arithmetic (tests/harness/cloud_cases.py) against the fixture (tests/golden/clouds.npz, the reference's own
outputs) bit for bit, the ctypes mirrors against include/ia3.h, and the stand-alone check of csrc/ia3_cloud.h
(tests/native/cloud_cpu.cpp), also under AddressSanitizer and UBSan."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import load_golden
from harness import cloud_cases as K

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def gold():
    return load_golden("clouds.npz")


@pytest.fixture(scope="module")
def V():
    from imageanalysis3_amd import visual_tools
    return visual_tools


@pytest.fixture(scope="module")
def S():
    from imageanalysis3_amd.structure_tools import chromosome
    return chromosome


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_names_and_signatures_are_the_references(V, S, gold):
    for name in ("gauss_ker", "add_source", "subtract_source", "plus_source"):
        assert str(inspect.signature(getattr(V, name))) == str(gold["sig_" + name]), name
    assert str(inspect.signature(S.convert_chr2Zxys_2_Cloud)) == str(gold["sig_convert_chr2Zxys_2_Cloud"])
    assert str(inspect.signature(V.add_sources)) == "(im_, pos, h, sig, size_fold=10, rounding=None)"
    ref = inspect.signature(S.convert_chr2Zxys_2_Cloud).parameters
    lst = inspect.signature(S.convert_chr2Zxys_list_2_Clouds).parameters
    assert list(lst)[0] == "chr2Zxys_list" and list(lst)[1:] == list(ref)[1:]
    assert all(lst[k].default == ref[k].default for k in list(ref)[1:])
    import imageanalysis3_amd.structure_tools as st
    assert st.chromosome is S and not hasattr(__import__("imageanalysis3_amd"), "figure_tools")
    with pytest.raises(ImportError):
        __import__("imageanalysis3_amd.figure_tools")


def test_errors_come_before_any_device_call(V, S):
    """Every call here is refused in Python: with a device none of them reaches it, without one none raises IA3Error."""
    im = K.base_image(np.float32)
    with pytest.raises(NotImplementedError):
        V.gauss_ker([2, 2], 16, [0, 0])
    with pytest.raises(NotImplementedError):
        V.gauss_ker([2, 2, 2], 16, [0, 0])
    with pytest.raises(ValueError):
        V.gauss_ker([2, 2, 2], 512, [0, 0, 0])
    with pytest.raises(ValueError):
        V.gauss_ker([2, 2, 2], -1, [0, 0, 0])
    with pytest.raises(TypeError):
        V.gauss_ker([2, 2, 2], 2.5, [0, 0, 0])
    for kw in (dict(pos=[np.nan, 1, 1]), dict(pos=[1, np.inf, 1]), dict(sig=[2, np.nan, 2]), dict(sig=[2, 2, np.inf]),
               dict(size_fold=np.inf), dict(sig=[409.7, 1, 1]), dict(sig=[-1, -1, -1]), dict(size_fold=-1)):
        with pytest.raises(ValueError):
            V.add_source(im, **kw)
    with pytest.raises(NotImplementedError):
        V.add_source(im[0], pos=[1, 1], sig=[2, 2])
    with pytest.raises(NotImplementedError):
        V.add_source(im[0])
    with pytest.raises(TypeError):
        V.add_source(im.astype(np.complex64))
    pos = np.zeros((4, 3))
    for args in ((np.zeros((4, 2)), 1, [2, 2, 2]), (pos, [1, 2, 3], [2, 2, 2]), (pos, 1, [2, 2]), (pos, 1, np.ones((3, 3)))):
        with pytest.raises(ValueError):
            V.add_sources(im, *args)
    with pytest.raises(ValueError):
        V.add_sources(im, pos, 1, [2, 2, 2], size_fold=[1, 2])
    with pytest.raises(ValueError):
        V.add_sources(im, pos, 1, [2, 2, 2], rounding=np.float16)
    cell = K.cell()
    with pytest.raises(TypeError):
        S.convert_chr2Zxys_2_Cloud([cell["c1"]])
    with pytest.raises(ValueError):
        S.convert_chr2Zxys_2_Cloud({"a": np.zeros((2, 5, 2))})
    with pytest.raises(ValueError):
        S.convert_chr2Zxys_2_Cloud({"a": np.zeros((5, 3))})
    for kw in (dict(pixel_size=0), dict(pixel_size=-0.1), dict(pixel_size=np.nan), dict(im_radius=np.inf), dict(gaussian_sigma=np.nan),
               dict(im_radius=0.01), dict(pixel_size=1e-4), dict(gaussian_sigma=300.0)):
        with pytest.raises(ValueError):
            S.convert_chr2Zxys_2_Cloud(cell, **kw)
    with pytest.raises(ValueError):
        S.convert_chr2Zxys_list_2_Clouds([cell, {"a": np.zeros((5, 3))}])
    with pytest.raises(ValueError):           # np.concatenate of nothing, as in the reference
        S.convert_chr2Zxys_2_Cloud({})
    # nothing kept: no device call is needed, with or without a device
    assert S.convert_chr2Zxys_2_Cloud({"gone": cell["gone"]}, **K.cloud_kwargs(K.cloud_options()[0])) == {}
    out = S.convert_chr2Zxys_list_2_Clouds([{"gone": cell["gone"]}], **K.cloud_kwargs(K.cloud_options()[4]))
    assert list(out[0]) == ["gone"] and same(out[0]["gone"], np.zeros((1, 12, 12, 12), dtype=np.float32))
    assert S.convert_chr2Zxys_list_2_Clouds([]) == []


def test_library_refuses_before_the_device_is_touched():
    """ia3_cloud_* check their arguments before they initialise the device: IA3_EINVAL with or without one."""
    from imageanalysis3_amd import _lib as L
    src = np.array([[1.0, 1, 1, 1, 2, 2, 2, 10]])
    start = np.array([0, 1], dtype=np.int32)
    out = np.zeros((1, 4, 4, 4))

    def rc(src=src, start=start, n=1, d=(4, 4, 4), mode=L.IA3_CLOUD_F64, out=out, dev=False):
        o = None if out is None else out.ctypes.data
        if dev:
            return L.lib().ia3_cloud_render_dev(None if src is None else L.ptr(src), None if start is None else L.ptr(start), n,
                                                d[0], d[1], d[2], mode, 1, o)
        return L.lib().ia3_cloud_render(None if src is None else L.ptr(src), None if start is None else L.ptr(start), n,
                                        d[0], d[1], d[2], mode, None, o)

    def row(**kw):
        r = src.copy()
        for k, v in kw.items():
            r[0, int(k[1:])] = v
        return r

    for dev in (False, True):
        for kw in (dict(src=None), dict(start=None), dict(out=None), dict(n=0), dict(n=65536), dict(mode=2), dict(d=(0, 4, 4)),
                   dict(d=(4, 4097, 4)), dict(start=np.array([1, 1], dtype=np.int32)), dict(start=np.array([0, 2, 1], dtype=np.int32), n=2),
                   dict(src=row(c0=np.nan)), dict(src=row(c2=np.inf)), dict(src=row(c5=np.nan)), dict(src=row(c7=-np.inf)),
                   dict(src=row(c4=409.7)), dict(src=row(c4=-1, c5=-1, c6=-1))):
            assert rc(dev=dev, **kw) == L.IA3_EINVAL, (dev, list(kw))
    sig, disp, ker = np.ones(3), np.zeros(3), np.zeros((2, 2, 2))
    assert L.lib().ia3_cloud_gauss_ker(None, 1, L.ptr(disp), L.ptr(ker)) == L.IA3_EINVAL
    assert L.lib().ia3_cloud_gauss_ker(L.ptr(sig), 1, None, L.ptr(ker)) == L.IA3_EINVAL
    assert L.lib().ia3_cloud_gauss_ker(L.ptr(sig), 1, L.ptr(disp), None) == L.IA3_EINVAL
    assert L.lib().ia3_cloud_gauss_ker(L.ptr(sig), -1, L.ptr(disp), L.ptr(ker)) == L.IA3_EINVAL
    assert L.lib().ia3_cloud_gauss_ker(L.ptr(sig), 512, L.ptr(disp), L.ptr(ker)) == L.IA3_EINVAL


def test_ctypes_mirrors_match_the_header():
    from imageanalysis3_amd import _lib
    src = open(os.path.join(ROOT, "include", "ia3.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    found = re.findall(r"\b(?:int|void)\s+(ia3_cloud_[a-z_]+)\s*\(", src)
    assert sorted(found) == sorted(e for e in _lib.EXPORTS if e.startswith("ia3_cloud_")) and len(found) == 3
    for name in ("IA3_CLOUD_F64", "IA3_CLOUD_F32", "IA3_CLOUD_MAX_S", "IA3_CLOUD_MAX_KER_S", "IA3_CLOUD_MAX_IMAGES", "IA3_CLOUD_MAX_DIM"):
        assert int(re.search(r"#define %s (\d+)" % name, src).group(1)) == getattr(_lib, name), name
    hdr = open(os.path.join(ROOT, "imageanalysis3_amd", "csrc", "ia3_cloud.h")).read()
    assert int(re.search(r"CL_S_MAX = (\d+)", hdr).group(1)) == _lib.IA3_CLOUD_MAX_S
    assert int(re.search(r"CL_KER_S_MAX = (\d+)", hdr).group(1)) == _lib.IA3_CLOUD_MAX_KER_S
    assert float(re.search(r"CL_CUT = (-\d+\.\d+)", hdr).group(1)) == -746.0
    assert issubclass(_lib.CloudImages, _lib.Owner)
    assert "free" not in vars(_lib.CloudImages) and "__del__" not in vars(_lib.CloudImages)


def test_source_table():
    from imageanalysis3_amd import _lib as L
    t = L.cloud_sources(np.arange(6).reshape(2, 3), 3, [1, 2, 3], 10)
    assert t.dtype == np.float64 and t.tolist() == [[0, 1, 2, 3, 1, 2, 3, 10], [3, 4, 5, 3, 1, 2, 3, 10]]
    t = L.cloud_sources(np.zeros((2, 3)), [1, -2], [[1, 2, 3], [4, 5, 6]], [7, 8])
    assert t[:, 3:].tolist() == [[1, 1, 2, 3, 7], [-2, 4, 5, 6, 8]]
    assert L.cloud_sources(np.zeros((0, 3)), 1, [1, 1, 1], 1).shape == (0, 8)
    assert L.cloud_sources(np.zeros((1, 3)), np.nan, [0, 0, 0], 10).shape == (1, 8)      # h and a zero sigma are free
    assert L.cloud_sources(np.zeros((1, 3)), 1, [409.6, 1, 1], 10).shape == (1, 8)       # a box of 4097
    assert L.cloud_sources(np.zeros((1, 3)), 1, [-0.05, -1, -1], 10).shape == (1, 8)     # int(-0.5) is 0


# ---- the NumPy restatement against the reference's outputs ------------------------------------------------------------------

def test_restatement_of_gauss_ker_equals_the_fixture(gold):
    for name, (sig, s, disp) in K.ker_cases().items():
        assert same(K.np_gauss_ker(sig, s, disp), gold[name]), name
    z = gold["ker_zero_sigma"]
    assert np.isnan(z[:, :, 3]).all() and (z[:, :, :3] == 0).all()
    # the pairing: another order of the same sigmas and displacements is another kernel
    sig, s, disp = K.ker_cases()["ker_s7"]
    for perm in ((0, 1, 2), (1, 2, 0), (2, 1, 0), (0, 2, 1), (1, 0, 2)):
        other = K.np_gauss_ker([sig[p] for p in perm], s, [disp[p] for p in perm])
        assert not np.allclose(other, gold["ker_s7"]) or perm == (0, 1, 2), perm


def test_restatement_of_add_source_equals_the_fixture(gold):
    cases = K.source_cases()
    assert len(cases) == 19 + 19 + 9
    touched = 0
    for name, (dtype, pos, h, sig, fold) in cases.items():
        base = K.base_image(dtype)
        out = gold[name]
        assert same(K.np_add_source(base, pos, h, sig, fold), out), name
        f = base.astype(np.float64)
        assert same(out[-1], f[-1]) and same(out[:, -1], f[:, -1]) and same(out[:, :, -1], f[:, :, -1]), name
        touched += int(not same(out, f))
        if "far" in name:
            assert same(out, f), name
    assert touched >= 25
    assert not same(gold["src_even_m050"], K.base_image(np.float32).astype(np.float64))      # -0.5 truncates to 0, not to -1
    pos, h, sig, fold = K.multi_case()
    im = K.base_image(np.float32)
    assert same(K.np_add_sources(im, pos, h, sig, fold), gold["multi_f64"])
    assert same(K.np_add_sources(im, pos, h, sig, fold, rounding=np.float32), gold["multi_f32"])
    assert not same(gold["multi_f64"].astype(np.float32), gold["multi_f32"])
    n = K.contributing(K.SHAPE, pos, sig, fold)
    assert n.max() >= 8 and (n[-1] == 0).all() and (n[:, -1] == 0).all() and (n[:, :, -1] == 0).all()
    pfit = np.array([150.0, 5.3, 4.6, 3.2, 100.0, 0.0, 0.0, 0.0, 0.6, 0.5, 0.4])
    u16 = K.base_image(np.uint16)
    assert same(K.np_add_source(u16, pfit[1:4], -pfit[0], pfit[-3:], 10), gold["pfit_minus"])
    assert same(K.np_add_source(u16, pfit[1:4], pfit[0], pfit[-3:], 10), gold["pfit_plus"])


def test_restatement_of_the_clouds_equals_the_fixture(gold):
    cell = K.cell()
    seen = set()
    for i, opt in enumerate(K.cloud_options()):
        out = K.np_cloud(cell, **K.cloud_kwargs(opt))
        assert ",".join(out) == str(gold["cloud_%d_keys" % i]), opt
        for c, arr in out.items():
            assert same(arr, gold["cloud_%d_%s" % (i, c)]), (opt, c)
            seen.add((c, len(arr)))
    # one, two and three homologs; the homolog with exactly MIN_SPOTS valid loci dropped and returned empty; the chromosome
    # that disappears at min_valid_per 0.3 and the one that always does
    assert {("c1", 1), ("c2", 2), ("c3", 3), ("few", 1), ("few", 2), ("per", 1), ("gone", 1)} <= seen
    assert "per" in str(gold["cloud_0_keys"]) and "per" not in str(gold["cloud_2_keys"]) and "gone" not in str(gold["cloud_1_keys"])
    assert not gold["cloud_3_few"][0].any() and gold["cloud_3_few"][1].any() and not gold["cloud_3_gone"].any()
    valid = np.isfinite(cell["few"]).all(2).sum(1)
    assert valid.tolist() == [K.MIN_SPOTS, K.MIN_SPOTS + 1] and np.isfinite(cell["per"]).all(2).mean() == 0.275


def test_restatement_of_the_default_size_cloud_equals_the_fixture(gold):
    big = K.np_cloud(K.default_cell())["1"]
    assert big.shape == (1, 100, 100, 100) and big.dtype == np.float32
    assert same(np.sum(big), gold["big_sum"])
    assert same(big.ravel()[K.sample_index(big.size)], gold["big_samples"])
    assert same(np.stack([big[0, -1], big[0, :, -1], big[0, :, :, -1]]), gold["big_planes"]) and not gold["big_planes"].any()


# ---- csrc/ia3_cloud.h on the host -------------------------------------------------------------------------------------------

SRC = os.path.join(HERE, "native", "cloud_cpu.cpp")
HDR = os.path.join(ROOT, "imageanalysis3_amd", "csrc", "ia3_cloud.h")
EXE = os.path.join(HERE, "native", "cloud_cpu")


def _build(exe, extra=()):
    if not os.path.isfile(exe) or os.path.getmtime(exe) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off"] + list(extra) + ["-o", exe, SRC])
    return exe


def _numpy_box(pos, sig, fold, shape):
    """The box of a source in NumPy's floating point, the way visual_tools.py:91-104 gets it (casts to int truncate, the
    half box is a float division) and not the integer way of cl_box: (s, first index before the clamp, lo, hi, fraction),
    or None where the library refuses the source."""
    v = max(sig) * fold
    if not (np.isfinite(sig).all() and np.isfinite(fold)) or not -1 < v < 4097:
        return None
    s = int(v)
    centre = np.asarray(pos, dtype=np.float64)
    whole = centre.astype(np.int64)                          # toward zero
    fraction = -whole + centre
    first = (whole - (s + 1) / 2).astype(np.int64)           # toward zero again
    last = first + (s + 1)
    top = np.asarray(shape, dtype=np.int64)
    lo, hi = (np.where(v >= top, top - 1, np.where(v < 0, 0, v)) for v in (first, last))
    return s, first, lo, hi, fraction


def _rows():
    rs = np.random.RandomState(27)
    sources = []
    for sig, fold in (K.SMALL_EVEN, K.SMALL_ODD, K.LARGE, ((1.0, 1.0, 1.0), 0), ((0.3, 0.2, 0.1), 5)):   # boxes of 4, 5, 21, 1, 2
        for _, pos in K.positions():
            sources.append((pos, sig, fold, K.SHAPE))
        for v in (-1.0, -0.999, -1e-9, 0.0, 0.999, 1.0, 1.5, 2.0, 2.5, 7.0, 7.5, 11.0, 11.999, 12.0, 12.5, 13.0, 13.5, 14.0, 1e12, -1e12):
            sources.append(((v, v, v), sig, fold, (12, 12, 12)))
    for _ in range(3000):
        shape = tuple(rs.randint(1, 40, 3))
        pos = rs.uniform(-8, np.array(shape) + 8.0)
        if rs.rand() < 0.3:
            pos = np.round(pos * 2) / 2
        sources.append((tuple(pos), tuple(rs.uniform(0.05, 3.0, 3)), float(rs.choice([1, 2.5, 6, 10, 15])), shape))
    for sig, fold in (((np.nan, 1, 1), 10), ((1, 1, np.inf), 10), ((1, 1, 1), np.inf), ((1, 1, 1), np.nan), ((409.7, 1, 1), 10),
                      ((409.6, 1, 1), 10), ((-1, -1, -1), 10), ((-0.05, -1, -1), 10), ((0.0, 0.0, 0.0), 10)):
        sources.append((K.BASE_POS, sig, fold, K.SHAPE))
    boxes = np.zeros((len(sources), 24))
    refused = 0
    for r, (pos, sig, fold, shape) in zip(boxes, sources):
        r[:3], r[3], r[4:7], r[7], r[8:11] = pos, 1.0, sig, fold, shape
        b = _numpy_box(pos, sig, fold, shape)
        if b is None:
            r[11] = -1
            refused += 1
        else:
            r[11], r[12:15], r[15:18], r[18:21], r[21:24] = b
    n = 8192
    coord = rs.randint(-60, 4200, n)
    disp = np.where(rs.rand(n) < 0.1, 0.0, rs.rand(n))
    s = rs.randint(0, 4097, n)
    sig = rs.uniform(0.05, 6.0, n)
    sig[:16] = 0.0
    coord[:8], disp[:8], s[:8] = 3, 0.0, 6            # 0 / 0
    ta, tb = rs.uniform(0, 50, n), rs.uniform(0, 900, n)
    ta[100:110] = np.inf
    with np.errstate(all="ignore"):
        u = ((coord - disp) - s / 2.) / sig**2
        term = u**2
        arg = -np.sum(np.stack([ta, tb, term], axis=-1), axis=-1) / 2.
    assert np.isnan(term[:8]).all() and np.isinf(term[8:16]).all()
    terms = np.stack([coord, disp, s, sig, term, ta, tb, arg], axis=1).astype(np.float64)
    return boxes, refused, terms


def _check(exe, tmp_path):
    boxes, refused, terms = _rows()
    assert refused == 6
    pb, pt = tmp_path / "boxes.f64", tmp_path / "terms.f64"
    np.ascontiguousarray(boxes).tofile(str(pb))
    np.ascontiguousarray(terms).tofile(str(pt))
    p = subprocess.run([exe, str(pb), str(pt)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(p.stdout[-3000:])
    assert p.returncode == 0, p.stdout[-2000:]
    m = re.search(r"boxes (\d+) mismatches (\d+)", p.stdout)
    assert m and int(m.group(1)) == len(boxes) and int(m.group(2)) == 0
    kept = boxes[boxes[:, 11] >= 0]
    m = re.search(r"empty (\d+)", p.stdout)
    assert m and int(m.group(1)) == int((kept[:, 18:21] <= kept[:, 15:18]).any(axis=1).sum()) > 100
    assert re.search(r"disp mismatches 0\b", p.stdout)
    m = re.search(r"terms (\d+) mismatches (\d+)", p.stdout)
    assert m and int(m.group(1)) == len(terms) == 8192 and int(m.group(2)) == 0
    assert "pairs 2 0 1" in p.stdout


def test_boxes_and_terms_on_the_host(tmp_path):
    _check(_build(EXE), tmp_path)


def test_boxes_and_terms_under_sanitizers(tmp_path):
    """the same stand-alone program with AddressSanitizer and UBSan (a host program of its own: nothing is preloaded)"""
    _check(_build(EXE + "_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]), tmp_path)
