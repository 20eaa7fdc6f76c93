"""Density clouds of traced chromosomes on the device (reference: structure_tools/chromosome.py).
``convert_chr2Zxys_2_Cloud`` (:5-57) turns every homolog of a traced nucleus into a float32 volume of
``int(im_radius*2/pixel_size)`` voxels along each axis: one Gaussian box per finite locus, pasted by ``visual_tools.add_source``
in a Python loop.  Here all kept homologs of a cell are one launch (``ia3_cloud_render``: cloud.hip)
in which every voxel gathers its loci in the reference's order and rounds to float32 after each, as the reference's
assignment into a float32 slice does.  The rules around the loop run here in NumPy as written there: the centring by one
``nanmean``, ``allowed_homolog_num``, the two validity thresholds, the two normalisations (NumPy's own sums and divisions on
the downloaded arrays) and the dropping of empty homologs and chromosomes.

``convert_chr2Zxys_list_2_Clouds`` walks a list of cells with one device allocation.  There is no CPU fallback.

All ``file:line`` citations are relative to the reference tree.
"""
import numpy as np

from .. import _lib as L


def _centre_of_cell(cell):
    """What figure_tools/plot_decode.py:110-120 subtracts from every chromosome: the ``nanmean`` over all loci of all homologs
    of all chromosomes of the cell, one value per axis (there is no figure_tools package here)."""
    loci = [np.asarray(zxys, dtype=np.float64) for homologs in cell.values() for zxys in homologs]
    return np.nanmean(np.concatenate(loci), axis=0)


class _Plan(object):
    """What one cell asks of the device: the source table of its kept homologs and where their images go."""

    def __init__(self, cell, pixel_size, im_radius, gaussian_sigma, allowed_homolog_num, min_valid_spots, min_valid_per):
        if not hasattr(cell, "items"):
            raise TypeError("chr2Zxys should be a dict chr -> homologs of (regions, 3) coordinates, got %s" % type(cell))
        for name, homologs in cell.items():
            for zxys in homologs:
                if np.ndim(zxys) != 2 or np.shape(zxys)[1] != 3:
                    raise ValueError("chr2Zxys[%r]: homologs of shape (regions, 3) are required, got %s" % (name, np.shape(zxys)))
        if not (np.isfinite(pixel_size) and pixel_size > 0 and np.isfinite(im_radius) and np.isfinite(gaussian_sigma)):
            raise ValueError("pixel_size > 0 and a finite im_radius and gaussian_sigma are required, got %r, %r and %r"
                             % (pixel_size, im_radius, gaussian_sigma))
        self.size = int(im_radius * 2 / pixel_size)                               # :18, voxels along an axis
        if self.size < 1 or self.size > L.IA3_CLOUD_MAX_DIM:
            raise ValueError("int(im_radius*2/pixel_size) = %d voxels along an axis (1 to %d)" % (self.size, L.IA3_CLOUD_MAX_DIM))
        centre = _centre_of_cell(cell)
        # :17-21 chromosomes with an allowed number of homologs, in the dict's order
        self.homologs = {name: len(homologs) for name, homologs in cell.items() if len(homologs) in allowed_homolog_num}
        sigma = np.full(3, gaussian_sigma / pixel_size)                           # :22, in voxels
        self.kept, tables, starts = [], [], [0]                                   # (chr, homolog, number of valid loci)
        for name in self.homologs:
            for i, zxys in enumerate(cell[name]):
                centred = np.asarray(zxys, dtype=np.float64) - centre
                valid = np.isfinite(centred).all(axis=1)
                n_valid = np.sum(valid)
                if n_valid <= min_valid_spots or np.mean(valid) < min_valid_per:  # :29, the homolog stays empty
                    continue
                pos = (im_radius + centred[valid]) / pixel_size                   # :34-37, finite loci only, in voxels
                tables.append(L.cloud_sources(pos, 1, sigma, im_radius * 3))      # :38-39
                starts.append(starts[-1] + len(pos))
                self.kept.append((name, i, n_valid))
        self.table = np.concatenate(tables) if tables else np.zeros((0, 8))
        self.image_start = np.array(starts, dtype=np.int32)
        self.nbytes = 4 * len(self.kept) * self.size**3

    def finish(self, images, normalize_counts, normalize_pdf, return_empty):
        """The dict the reference returns, from the rendered images of the kept homologs: the two normalisations (:40-45,
        NumPy's own division of the float32 image by the int64 count and by its float32 ``np.sum``, stored as float32) and,
        unless ``return_empty``, without the homologs that are zero everywhere and the chromosomes that keep none (:47-55)."""
        clouds = {name: np.zeros((H,) + (self.size,) * 3, dtype=np.float32) for name, H in self.homologs.items()}
        for (name, i, n_valid), im in zip(self.kept, images):
            row = clouds[name][i]          # a view: assigning into it rounds to float32
            row[...] = im
            if normalize_counts:
                row[...] = row / n_valid
            if normalize_pdf:
                row[...] = row / np.sum(row)
        if return_empty:
            return clouds
        out = {}
        for name, arr in clouds.items():
            filled = arr.reshape(len(arr), -1).any(axis=1)
            if filled.any():
                out[name] = arr[filled]
        return out


def convert_chr2Zxys_2_Cloud(chr2Zxys,
                             pixel_size=0.1, im_radius=5,
                             gaussian_sigma=0.5,
                             allowed_homolog_num=[1,2],
                             min_valid_spots=20, min_valid_per=0.25,
                             normalize_counts=False, normalize_pdf=False,
                             return_empty=False,
                             ):
    """:5-57 ``chr -> (homologs, size, size, size)`` float32 density clouds of a cell ``chr -> (homologs, regions, 3)``."""
    plan = _Plan(chr2Zxys, pixel_size, im_radius, gaussian_sigma, allowed_homolog_num, min_valid_spots, min_valid_per)
    images = []
    if len(plan.kept):
        images = L.cloud_render(plan.table, plan.image_start, (plan.size,)*3, rounding=np.float32)
    return plan.finish(images, normalize_counts, normalize_pdf, return_empty)


def convert_chr2Zxys_list_2_Clouds(chr2Zxys_list,
                                   pixel_size=0.1, im_radius=5,
                                   gaussian_sigma=0.5,
                                   allowed_homolog_num=[1,2],
                                   min_valid_spots=20, min_valid_per=0.25,
                                   normalize_counts=False, normalize_pdf=False,
                                   return_empty=False,
                                   ):
    """``[convert_chr2Zxys_2_Cloud(cell, ...) for cell in chr2Zxys_list]`` with the device memory of the largest cell
    allocated once.  Every cell is checked before the first device call."""
    plans = [_Plan(_cell, pixel_size, im_radius, gaussian_sigma, allowed_homolog_num, min_valid_spots, min_valid_per)
             for _cell in chr2Zxys_list]
    out = []
    if not any(len(p.kept) for p in plans):
        return [p.finish([], normalize_counts, normalize_pdf, return_empty) for p in plans]
    with L.CloudImages(max(p.nbytes for p in plans)) as buf:
        for p in plans:
            images = buf.render(p.table, p.image_start, (p.size,)*3, rounding=np.float32) if len(p.kept) else []
            out.append(p.finish(images, normalize_counts, normalize_pdf, return_empty))
    return out
