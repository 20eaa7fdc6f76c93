"""Fixtures of the compartment densities: tests/golden/compartment_density.npz.

Runs the reference's own ``compartment_tools/density.py`` (``calculate_compartment_densities`` and
``calculate_gaussian_density``) on the cases of tests/harness/density_cases.py.  The module is loaded by file as
oracle/ref_loader.py loads the others.  Only outputs are stored:

    small_<options>, large_<options>   (2, points) float64: the A and B densities of the cells with the full option matrix
                                       and of the larger cells (four option sets), in the population's point order
    smallcnt_<flags>, largecnt_<flags> (2, points) int32: the rows the reference adds up per query (the same run with a
                                       Gaussian term of 1 for every row), -1 where it gives NaN
    gauss_<i>                          calculate_gaussian_density of the (sigma, intensity, background) triple i
    arg_t                              -0.5 * np.sum((c - q)**2 / sigma**2, axis=-1) of density_cases.arg_case()
    sig_<name>                         str(inspect.signature) of the three reference functions

Needs the reference tree (IA3_REFERENCE); nothing here runs on the GPU.  ``BatchCompartmentDensities`` is the same
function per cell in a process pool and is not run.

    python scripts/make_density_golden.py

The script asserts the facts about NumPy's arithmetic that csrc/ia3_density.h is built on.
"""
import importlib.util
import inspect
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

OUT = os.path.join(ROOT, "tests", "golden")


def load_module():
    import ref_loader
    spec = importlib.util.spec_from_file_location("IA3_compartment_density",
                                                  os.path.join(ref_loader.REF, "compartment_tools", "density.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def same(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def facts(ref, K):
    """The order of the three-term sum, x**2 as x * x, the zero cut and the sign of the difference."""
    v = K.arg_case()
    c, q, s = v[:, :3], v[:, 3:6], v[:, 6:]
    s2 = s**2
    with np.errstate(all="ignore"):
        t = -0.5 * np.sum((c - q)**2 / s2, axis=-1)
        d = c - q
        mine = -0.5 * ((d[:, 0] * d[:, 0] / s2[:, 0] + d[:, 1] * d[:, 1] / s2[:, 1]) + d[:, 2] * d[:, 2] / s2[:, 2])
        other = -0.5 * (d[:, 0] * d[:, 0] / s2[:, 0] + (d[:, 1] * d[:, 1] / s2[:, 1] + d[:, 2] * d[:, 2] / s2[:, 2]))
        assert same(t, mine) and not same(t, other)
        flipped = -0.5 * np.sum((q - c)**2 / s2, axis=-1)
        assert same(t, flipped)
        assert same(ref.calculate_gaussian_density(c, q, s), np.exp(t))
    assert same(s2, s * s)
    assert np.exp(-746.0) == 0.0 and np.exp(-745.0) > 0.0 and np.exp(-np.inf) == 0.0
    assert np.isnan(t[129]) and t[128] == -np.inf and t[130] == -np.inf and np.isnan(t[131])
    return t


def main():
    from harness import density_cases as K
    ref = load_module()
    warnings.simplefilter("ignore")
    d = {"arg_t": facts(ref, K)}
    cells = K.cells()
    real = ref.calculate_gaussian_density

    def run(indices, opt, ones=False):
        c, t, x, n, s = opt
        ref.calculate_gaussian_density = (lambda zxys, zxy, r: np.ones(len(zxys))) if ones else real
        try:
            out = [ref.calculate_compartment_densities(cells[i], K.AB, K.SIGMAS[s], normalize_by_reg_num=bool(n),
                                                       exclude_self=bool(x), use_cis=bool(c), use_trans=bool(t)) for i in indices]
        finally:
            ref.calculate_gaussian_density = real
        for i, o in zip(indices, out):
            assert list(o) == list(cells[i]) and all(o[c_]['A'].shape == cells[i][c_].shape[:2] for c_ in o)
        return K.flat(out)

    for tag, indices, options in (("small", K.small_indices(), K.full_options()), ("large", K.large_indices(), K.LARGE_OPTIONS)):
        for opt in options:
            d["%s_%s" % (tag, K.option_name(*opt))] = run(indices, opt)
            key = "%scnt_c%dt%dx%d" % (tag, opt[0], opt[1], opt[2])
            if key not in d:
                cnt = run(indices, opt[:3] + (0, opt[4]), ones=True)
                assert (np.isnan(cnt) | (cnt == np.round(cnt))).all()
                d[key] = np.where(np.isnan(cnt), -1, cnt).astype(np.int32)
        print(tag, "points", d["%s_%s" % (tag, K.option_name(*options[0]))].shape[1], "option sets", len(options))
    # the far cell under trans alone: terms in the subnormal band and below the zero cut, and some above it
    far = run([len(cells) - 1], (0, 1, 1, 0, "scalar"))
    assert (far == 0).any() and ((far > 0) & (far < 2.3e-308)).any() and (far > 2.3e-308).any(), far
    centers, rc, triples = K.gaussian_case()
    for i, (sigma, intensity, background) in enumerate(triples):
        d["gauss_%d" % i] = ref.calculate_gaussian_density(centers, rc, sigma, intensity, background)
    for name in ("calculate_gaussian_density", "calculate_compartment_densities", "BatchCompartmentDensities"):
        d["sig_" + name] = np.array(str(inspect.signature(getattr(ref, name))))
    d["source"] = np.array("reference")
    path = os.path.join(OUT, "compartment_density.npz")
    np.savez_compressed(path, **d)
    print("arrays", len(d), "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
