"""Fixtures of the chromosome image: tests/golden/chromim.npz.

Runs the reference's own ``Field_of_View._generate_chrom_im_from_data`` (classes/field_of_view.py:1821-1917) on the two
small save files of tests/harness/chromim_cases.py.  The module is loaded file by file as oracle/ref_loader.py loads the
others; the method is called on a stand-in ``self`` that carries the four attributes it reads.  Stand-ins: ``h5py`` is
backed by this package's ``io_tools.h5lite`` (plus the boolean-mask read of ``_grp['ids'][_flags > 0]``),
``load_image_from_fov_file`` is this package's (tests/test_h5_cpu.py pins it against the reference's), the multiprocessing
reducer the module installs on import is left out, and ``scipy.ndimage.interpolation`` (gone from current SciPy) is
``scipy.ndimage``.  ``find_image_background`` of the ``_fast=False`` pass is the reference's own.  Only the outputs are
stored; the tests write the files again.  Needs the reference tree (IA3_REFERENCE) and libhdf5; nothing here runs on the
GPU.

    python scripts/make_chrom_image_golden.py

The script asserts what the tests rely on: that tests/harness/chromim_ref.py reproduces every stored array byte for byte.
"""
import multiprocessing.reduction
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

OUT = os.path.join(ROOT, "tests", "golden")


class _Dataset(object):
    def __init__(self, ds):
        self._ds = ds

    def __getitem__(self, key):
        if isinstance(key, np.ndarray) and key.dtype == bool:
            return self._ds[...][key]
        return self._ds[key]


class _Group(object):
    def __init__(self, grp):
        self._grp = grp

    def __getitem__(self, name):
        return _Dataset(self._grp[name])


class _File(object):
    def __init__(self, *a, **kw):
        from imageanalysis3_amd.io_tools import h5lite
        self._f = h5lite.File(*a, **kw)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self._f.close()
        return False

    def __getitem__(self, name):
        return _Group(self._f[name])


def load_field_of_view():
    """The reference's classes/field_of_view.py with the stand-ins above; returns (module, reference io_tools.load)."""
    import ref_loader
    import scipy.ndimage
    from imageanalysis3_amd.classes import batch_functions as B
    from imageanalysis3_amd.classes import _allowed_kwds, _max_num_seeds, _min_num_seeds
    ns = ref_loader.load_reference()
    io_load, _ = ref_loader.load_io()
    sys.modules["h5py"] = types.ModuleType("h5py")
    sys.modules["h5py"].File = _File
    sys.modules.setdefault("scipy.ndimage.interpolation", scipy.ndimage)
    req = types.ModuleType("IA3.required_files")
    req.__path__ = []
    p2r = types.ModuleType("IA3.required_files.pickle2reducer")
    p2r.Pickle2Reducer = lambda: multiprocessing.reduction   # the context keeps its own reducer
    req.pickle2reducer = p2r
    sys.modules.update({"IA3.required_files": req, "IA3.required_files.pickle2reducer": p2r})
    cl = sys.modules["IA3.classes"]
    cl._allowed_kwds, cl._max_num_seeds, cl._min_num_seeds = _allowed_kwds, _max_num_seeds, _min_num_seeds
    cl._spot_seeding_th = 200
    bf = types.ModuleType("IA3.classes.batch_functions")
    bf.load_image_from_fov_file = B.load_image_from_fov_file
    sys.modules["IA3.classes.batch_functions"] = bf
    fov = ns._load("IA3.classes.field_of_view", ref_loader.REF + "/classes/field_of_view.py")
    return fov, io_load


def main():
    from harness import chromim_cases as K
    from harness import chromim_ref as R
    from imageanalysis3_amd.classes import batch_functions as B
    from imageanalysis3_amd.classes import _allowed_kwds
    fov, io_load = load_field_of_view()
    d = {}
    with tempfile.TemporaryDirectory() as tmp:
        for key in K.FILES:
            shape, data_type, batch, ids, slots = K.file_layout(key)
            path = os.path.join(tmp, key + ".hdf5")
            ims, fl, dr = K.write_file(B, path, key)
            for fast in (True, False):
                me = types.SimpleNamespace(shared_parameters={'allowed_data_types': _allowed_kwds, 'single_im_size': list(shape)},
                                           save_filename=path, image_dtype=np.uint16)
                got = fov.Field_of_View._generate_chrom_im_from_data(me, data_type, _num_loaded_image=batch, _fast=fast,
                                                                     _verbose=False)
                assert got.dtype == np.float64 and got.shape == shape and me.chrom_im is got
                want = R.chrom_im(ims, fl, dr, shape, fast=fast, background=io_load.find_image_background)
                assert want.tobytes() == got.tobytes(), (key, fast)
                if fast:
                    assert R.shifted_sum(ims, fl, dr, shape).tobytes() == got.tobytes(), key
                d["%s_%s" % (key, "fast" if fast else "slow")] = got
                if not fast:
                    d[key + "_cvals"] = np.array([io_load.find_image_background(im) for im in ims], dtype=np.float64)
    d["source"] = np.array("reference")
    path = os.path.join(OUT, "chromim.npz")
    np.savez_compressed(path, **d)
    print("arrays", sorted(d), "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
