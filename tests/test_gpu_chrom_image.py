"""GPU: the chromosome image on the device (csrc/chromim.hip) and find_candidate_chromosomes on it in float64
(csrc/morph.hip) against the statements tests/harness/chromim_ref.py and chromseg_ref.py and the reference's own outputs
(tests/golden/chromim.npz).  Every comparison is byte-exact."""
import numpy as np
import pytest

from conftest import load_golden
from harness import chromim_cases as K
from harness import chromim_ref as R
from harness import chromseg_ref as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from imageanalysis3_amd import _lib
    _lib.check(_lib.lib().ia3_init(0))
    return _lib


@pytest.fixture(scope="module")
def F(L):
    from imageanalysis3_amd.classes import field_of_view
    return field_of_view


@pytest.fixture(scope="module")
def CH(L):
    from imageanalysis3_amd.segmentation_tools import chromosome
    return chromosome


@pytest.fixture(scope="module")
def gold():
    return load_golden("chromim.npz")


@pytest.fixture(scope="module")
def rounds():
    """(images, flags, drifts, statement) of every shape and count, made once"""
    out = {}
    for name, shape in K.SHAPES.items():
        for count in K.COUNTS:
            ims, fl, dr = K.case(name, count)
            out[name, count] = (ims, fl, dr, R.chrom_im(ims, fl, dr, shape))
    return out


@pytest.fixture(scope="module")
def candidate_images():
    """name -> (images, flags, drifts, the statement's float64 chromosome image)"""
    out = {}
    for name in K.CANDIDATES:
        ims, fl, dr = K.round_copies(name)
        out[name] = (ims, fl, dr, R.chrom_im(ims, fl, dr, ims[0].shape))
    return out


def same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


# ---- medians ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(K.SHAPES))
def test_stack_median_equals_np_median(L, name):
    shape = K.SHAPES[name]
    images = dict(K.median_images(shape), generated=K.image(shape, 0))
    stacks = []
    for key, im in images.items():
        with L.DeviceStack.upload(im) as s:
            got = L.stack_median(s)
        want = np.median(im)
        assert type(got) is np.float64 and got.tobytes() == np.float64(want).tobytes(), (key, got, want)
    f32 = (images["generated"].astype(np.float32) / np.float32(3)).astype(np.float32)
    with L.DeviceStack.upload(f32) as s:
        assert L.stack_median(s) == np.float64(np.median(f32))
    # the medians the add uses are the same ones
    keys = sorted(images)
    with L.ChromImage.empty(shape) as c:
        stacks = [L.DeviceStack.upload(images[k]) for k in keys]
        try:
            bg = c.add(stacks, [1] * len(keys), np.zeros((len(keys), 3), int))
        finally:
            for s in stacks:
                s.free()
        assert bg.tolist() == [float(np.median(images[k])) for k in keys]
        assert same(c.download(), np.sum([images[k].astype(np.float64) for k in keys], axis=0))


# ---- the fast path ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", K.COUNTS)
@pytest.mark.parametrize("name", sorted(K.SHAPES))
def test_generate_chrom_im_equals_the_statement(L, F, rounds, gold, name, count):
    ims, fl, dr, want = rounds[name, count]
    got = F.generate_chrom_im(ims, fl, dr)
    assert same(got, want)
    stacks = [L.DeviceStack.upload(im) for im in ims]
    try:
        with F.generate_chrom_im(stacks, fl, dr, single_im_size=K.SHAPES[name], return_device=True) as dev:
            assert isinstance(dev, L.ChromImage) and dev.shape == K.SHAPES[name]
            assert same(dev.download(), want)
        assert same(F.generate_chrom_im(stacks, fl, dr), want)            # a second run: the same bytes
        for s, im in zip(stacks, ims):
            assert same(s.download(), im)                                 # the rounds are only read
    finally:
        for s in stacks:
            s.free()
    for key, (gname, gcount, _, _) in K.FILES.items():
        if (gname, gcount) == (name, count):
            assert same(got, gold[key + "_fast"])


def test_generate_chrom_im_continues_an_image(L, F, rounds):
    ims, fl, dr, want = rounds["small", 23]
    with L.ChromImage.empty(K.SHAPES["small"]) as dev:
        back = F.generate_chrom_im(ims[:10], fl[:10], dr[:10], chrom_im=dev, return_device=True)
        assert back is dev
        assert same(dev.download(), R.chrom_im(ims[:10], fl[:10], dr[:10], K.SHAPES["small"]))
        out = F.generate_chrom_im(ims[10:], fl[10:], dr[10:], chrom_im=dev)
        assert same(out, want) and same(dev.download(), want)             # still the caller's, still alive
    up = L.ChromImage.upload(want)
    try:
        assert same(up.download(), want)
        assert same(F.generate_chrom_im([], [], [], chrom_im=up), want)
    finally:
        up.free()


@pytest.mark.parametrize("key", sorted(K.FILES))
def test_generate_chrom_im_from_data(L, F, gold, tmp_path, capsys, key):
    from imageanalysis3_amd.classes import batch_functions as B
    shape, data_type, batch, ids, slots = K.file_layout(key)
    path = str(tmp_path / (key + ".hdf5"))
    ims, fl, dr = K.write_file(B, path, key)
    assert len(ids) == len(ims) + 2                                       # two ids with flag 0 among them
    want = R.chrom_im(ims, fl, dr, shape)
    capsys.readouterr()
    got = F.generate_chrom_im_from_data(path, data_type, num_loaded_image=batch)
    text = capsys.readouterr().out
    assert same(got, want) and same(got, gold[key + "_fast"])
    assert "- Generate chromosome image from %s images, %d images planned to load." % (data_type, len(ims)) in text
    assert text.count("-- shifting images in ") == -(-len(ims) // batch) and "-- finish generating chrom_im in " in text
    with F.generate_chrom_im_from_data(path, data_type, num_loaded_image=batch, return_device=True, verbose=False) as dev:
        assert same(dev.download(), want)
    assert capsys.readouterr().out == ""
    slow = F.generate_chrom_im_from_data(path, data_type, num_loaded_image=batch, fast=False, verbose=False)
    assert same(slow, gold[key + "_slow"])


# ---- the interpolating path ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(K.SHAPES))
def test_slow_path_equals_ndimage_shift(L, F, name):
    from imageanalysis3_amd.io_tools.load import find_image_background
    shape = K.SHAPES[name]
    ims, fl, dr = K.slow_case(name)
    want = R.chrom_im(ims, fl, dr, shape, fast=False, background=find_image_background)
    assert same(F.generate_chrom_im(ims, fl, dr, fast=False), want)
    cval = find_image_background(ims[4])
    only = R.chrom_im(ims[4:], fl[4:], dr[4:], shape, fast=False, background=find_image_background)
    assert (only == np.uint16(cval + 0.5)).all()                          # the drift beyond the axis: all cval
    assert same(F.generate_chrom_im(ims[4:], fl[4:], dr[4:], fast=False), only)


# ---- errors ----------------------------------------------------------------------------------------------------------------------
def test_errors(L, F):
    shape = K.SHAPES["odd"]
    ims, fl, dr = K.case("odd", 10)
    for axis in range(3):
        for d in (shape[axis], -shape[axis], shape[axis] + 3):
            bad = np.zeros((1, 3), np.float32)
            bad[0, axis] = d
            with pytest.raises(ValueError, match="broadcast"):
                F.generate_chrom_im(ims[:1], [1], bad)
            with L.ChromImage.empty(shape) as c, L.DeviceStack.upload(ims[0]) as s:
                with pytest.raises(ValueError, match="broadcast"):
                    c.add([s], [1], bad.astype(int))                      # the library refuses it too
                assert c.add([s], [2], bad.astype(int)).tolist() == [0.0]  # a warped image's drift is not read
                assert same(c.download(), ims[0].astype(np.float64))
    with pytest.raises(NotImplementedError):
        F.generate_chrom_im([ims[0].astype(np.float32)], [1], dr[:1])
    with L.ChromImage.empty(shape) as c:
        with L.DeviceStack.upload(ims[0].astype(np.float32)) as s, pytest.raises(NotImplementedError):
            c.add([s], [1], [[0, 0, 0]])
        with L.DeviceStack.upload(ims[0][:, :, :-1]) as s, pytest.raises(ValueError):
            c.add([s], [1], [[0, 0, 0]])
        assert not c.download().any()                                     # nothing was added


# ---- candidates in float64 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,name,kind,fs,per", K.candidate_cases(), ids=[c[0] for c in K.candidate_cases()])
def test_candidates_of_a_chromosome_image(L, F, CH, candidate_images, key, name, kind, fs, per):
    ims, fl, dr, total = candidate_images[name]
    if kind == "sum":
        stacks = [L.DeviceStack.upload(im) for im in ims]
        try:
            dev = F.generate_chrom_im(stacks, fl, dr, return_device=True)
        finally:
            for s in stacks:
                s.free()
        image = total
    else:
        image = total / 7
        dev = L.ChromImage.upload(image)
        with pytest.raises(NotImplementedError, match="exact in float32"):
            CH.find_candidate_chromosomes(image, _filt_size=fs, _binary_per_th=per, _verbose=False)
    st = S.chain(image, fs, per, 1, K.CAND_MIN_SIZE)
    assert len(st["ids"]) >= 3 and len(st["ids"]) < st["n"]
    with dev:
        assert same(dev.download(), image)
        coords, kept = CH.find_candidate_chromosomes(dev, _filt_size=fs, _binary_per_th=per, _min_label_size=K.CAND_MIN_SIZE,
                                                     _verbose=False, _return_label=True)
        with kept:
            assert same(kept.download(), st["kept_label"])
        assert same(coords, st["coords"])
        again, th, none = L.find_candidate_chromosomes(dev, fs, per, 1, K.CAND_MIN_SIZE)
        assert none is None and same(again, st["coords"])
        assert type(th) is np.float64 and th.tobytes() == np.float64(st["threshold"]).tobytes()
        assert same(CH.find_candidate_chromosomes(dev, _filt_size=fs, _binary_per_th=per, _min_label_size=K.CAND_MIN_SIZE,
                                                  _verbose=False), st["coords"])
        assert same(dev.download(), image)                                # the image is only read


def test_float64_front_refuses_what_the_other_fronts_refuse(L, CH, candidate_images):
    total = candidate_images["small"][3]
    zero = total.copy()
    zero[3, :, :40] = 0                                                   # more than half of plane 3
    with L.ChromImage.upload(zero) as dev:
        with pytest.raises(ValueError, match="plane 3"):
            CH.find_candidate_chromosomes(dev, _verbose=False)
    bad = total.copy()
    bad[5, 0, 0] = np.nan
    with L.ChromImage.upload(bad) as dev:
        with pytest.raises(ValueError, match="plane 5"):
            CH.find_candidate_chromosomes(dev, _verbose=False)
    with L.ChromImage.upload(total) as dev:
        for fsz in (0, 6):
            with pytest.raises(NotImplementedError, match="_filt_size"):
                CH.find_candidate_chromosomes(dev, _filt_size=fsz, _verbose=False)
        with pytest.raises(NotImplementedError, match="_morphology_size"):
            CH.find_candidate_chromosomes(dev, _morphology_size=2, _verbose=False)
