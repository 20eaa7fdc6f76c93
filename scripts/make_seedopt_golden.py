"""Fixtures of the seeding options: tests/golden/seedopt.npz.

Runs the reference's own spot_tools/fitting.py:20-154 ``get_seeds`` (loaded through oracle/ref_loader.py) on the main field
of tests/harness/seedopt_cases.py, float32 and uint16, for every case of ``seedopt_cases.golden_cases()``: ``filt_size``
1..8 with the front filter off and at 0.75, ``hot_pixel_th`` 0..6, ``min_edge_distance`` 0..13, the background widths at
the switch points of the lazy path and off, and one dynamic threshold that settles on a middle level.  Only outputs are
stored: per table the coordinates as int16 and the heights as float32 (both exact: asserted), the level the dynamic case
settled on, and the CRC of every stack.  Needs the reference tree (IA3_REFERENCE); nothing here runs on the GPU.

    python scripts/make_seedopt_golden.py

The script asserts what the tests rely on: that oracle/np_oracle.py::get_seeds reproduces every table byte for byte, also
for the cases that are not stored (front width 1.0, the ragged field, the noise stack), and the conditions of
``seedopt_cases.check_discrimination`` on the reference's tables.
"""
import contextlib
import io
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

OUT = os.path.join(ROOT, "tests", "golden")


def main():
    import ref_loader
    import np_oracle as O
    from harness import seedopt_cases as K
    fit = ref_loader.load_reference().fitting

    def ref(im, **kw):
        with contextlib.redirect_stdout(io.StringIO()):
            got = fit.get_seeds(np.array(im), return_h=True, **kw)
        ora = O.get_seeds(np.array(im), return_h=True, **kw)
        assert got.dtype == ora.dtype and got.shape == ora.shape and got.tobytes() == ora.tobytes(), kw
        return got

    d = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for dt in K.DTYPES:
            for name in ("main", "ragged", "noise"):
                d["crc_%s_%s" % (name, dt)] = np.uint32(K.crc(K.stack(name, dt)))
            for key, (name, kw) in K.golden_cases().items():
                zxy, h = K.table_i16(ref(K.stack(name, dt), **kw))
                d["%s_%s_zxy" % (dt, key)], d["%s_%s_h" % (dt, key)] = zxy, h
            with contextlib.redirect_stdout(io.StringIO()):
                _, th = O.get_seeds(np.array(K.stack("main", dt)), return_h=True, return_th=True, **K.DYNAMIC)
            level = int(round((1 - th / K.DYNAMIC["th_seed"]) * K.DYNAMIC["dynamic_niters"]))
            assert level == K.DYNAMIC_LEVEL, level
            d["%s_dynamic_level" % dt] = np.int32(level)
            K.check_discrimination(dt, lambda name, **kw: ref(K.stack(name, dt), **kw))   # oracle = reference inside
            print(dt, "tables", len(K.golden_cases()))
    d["source"] = np.array("reference")
    path = os.path.join(OUT, "seedopt.npz")
    # fixed order and timestamps: the file is the same bytes on every run
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for key in sorted(d):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(d[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())
    print("arrays", len(d), "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
