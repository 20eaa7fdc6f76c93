"""A/B compartment densities of traced cells on the device (reference: compartment_tools/density.py).
``calculate_compartment_densities`` (:11-87) gives every traced locus of a nucleus the sum of
``exp(-0.5 * sum((c - ref)**2 / sigma**2))`` over the A loci and over the B loci of the nucleus' other chromosome copies
(``use_trans``) and / or of its own copy (``use_cis``); ``BatchCompartmentDensities`` (:90-102) does so for a list of cells
in a process pool.  Here the loci of all cells are uploaded once (``_lib.DensityPopulation``) and every set of labels,
radii and flags is one library call (``ia3_density_scores_dev``): one lane per query, all pairs of a cell.
The argument of ``exp`` is NumPy's bit for bit; ``exp`` is the device's float64 one, so a sum agrees with the reference's
to 1e-12 relative (derived in §25), NaN for NaN.

``population_compartment_densities`` is the flat form on a resident population, for callers that repeat with shuffled
labels or other radii.  Indices of ``chr_2_AB_dict`` outside ``0..R-1`` raise ``IndexError`` (the reference wraps negative
ones for trans and drops them for cis).  There is no CPU fallback.

All ``file:line`` citations are relative to the reference tree.
"""
import numpy as np

from .. import _lib as L


def _squared_sigma(sigma):
    """:6-7 ``np.array(sigma, dtype=float)**2`` as three values (a scalar or one value per axis)."""
    s2 = np.array(sigma, dtype=float)**2
    if s2.ndim > 1 or (s2.ndim == 1 and s2.shape[0] not in (1, 3)):
        raise ValueError("sigma: a scalar or three values are required, got shape %s" % (s2.shape,))
    return np.ascontiguousarray(np.broadcast_to(s2, (3,)), dtype=np.float64)


def calculate_gaussian_density(centers, ref_center, sigma,
                               intensity=1, background=0):
    """:4-9 ``intensity * exp(-0.5 * sum((centers - ref_center)**2 / sigma**2, axis=-1)) + background`` for centres of
    shape (..., 3): every centre is a query of the density kernel with ``ref_center`` as its one contributor (the square
    does not see the sign of the difference), so the terms come back unsummed.  A NaN in ``ref_center`` makes every term
    NaN as in the reference; an infinite ``ref_center`` raises ``ValueError`` (the kernel drops such a contributor)."""
    s2 = _squared_sigma(sigma)
    c = np.asarray(centers, dtype=np.float64)
    ref = np.asarray(ref_center, dtype=np.float64)
    if c.ndim < 1 or c.shape[-1] != 3 or ref.shape != (3,):
        raise ValueError("calculate_gaussian_density: centers of shape (..., 3) and a ref_center of 3 values are required, got "
                         "%s and %s" % (c.shape, ref.shape))
    flat = c.reshape(-1, 3)
    if np.isnan(ref).any() or len(flat) == 0:
        g = np.full(c.shape[:-1], np.nan)
    elif not np.isfinite(ref).all():
        raise ValueError("calculate_gaussian_density: an infinite ref_center is not built")
    else:
        # cells of at most IA3_DENSITY_MAX_CELL points: a share of the centres as homolog 0 and the reference as homolog 1
        step = L.IA3_DENSITY_MAX_CELL - 1
        cells = [{'c': flat[i:i + step][None], 'r': ref[None, None]} for i in range(0, len(flat), step)]
        layout = L.DensityLayout(cells, ['c', 'r'])
        mult = layout.multiplicities({'c': {'A': [], 'B': []}, 'r': {'A': [0], 'B': []}})
        with L.DensityPopulation.upload(layout, None) as pop:
            sums, _ = pop.scores(mult, s2, use_cis=False, use_trans=True, exclude_self=False)
        g = np.concatenate([sums[0, at:at + H * R] for blocks in layout.blocks for ch, H, R, at in blocks if ch == 'c'])
        g = g.reshape(c.shape[:-1])
    g_pdf = float(intensity) * g + float(background)
    return g_pdf


def population_compartment_densities(population, chr_2_AB_dict, gaussian_radius,
                                     normalize_by_reg_num=False, exclude_self=True,
                                     use_cis=False, use_trans=True, return_counts=False):
    """The densities of every locus of a resident ``_lib.DensityPopulation`` as a (2, n_points) float64 array, row 0 for A
    and row 1 for B, in the population's point order (``population.layout.unpack`` makes the reference's dicts of it).
    Only the labels' multiplicities, three squared sigmas and the flags go to the device.  ``return_counts``: also the
    (2, n_points) int32 numbers of contributing rows."""
    if not use_cis and not use_trans:
        raise ValueError(f"One of use_cis or use_trans should be true!")
    layout = population.layout
    mult = layout.multiplicities(chr_2_AB_dict)
    s2 = _squared_sigma(gaussian_radius)
    sums, counts = population.scores(mult, s2, use_cis=use_cis, use_trans=use_trans, exclude_self=exclude_self)
    if normalize_by_reg_num:
        with np.errstate(invalid="ignore", divide="ignore"):
            sums = sums / counts          # :68 .mean(): 0 / 0 is NaN where no finite row is left
    if not use_cis:
        # :61 nothing was collected: trans alone in a cell that holds a single copy
        alone = np.repeat(layout.n_copies < 2, np.diff(layout.cell_start))
        sums[:, alone] = np.nan
    return (sums, counts) if return_counts else sums


def BatchCompartmentDensities(chr_2_zxys_dicts, chr_2_AB_dict, gaussian_radius,
                              num_threads=12,
                              normalize_by_reg_num=True, exclude_self=True,
                              use_cis=False, use_trans=True):
    """:90-102 the list of per-cell dicts ``chr -> {'A': (H, R), 'B': (H, R)}`` in one upload and one scoring call;
    ``num_threads`` is accepted and ignored."""
    if not use_cis and not use_trans:
        raise ValueError(f"One of use_cis or use_trans should be true!")
    cells = list(chr_2_zxys_dicts)
    layout = L.DensityLayout(cells, chr_2_AB_dict)
    layout.multiplicities(chr_2_AB_dict)       # the labels' errors before any device call
    _squared_sigma(gaussian_radius)
    if len(cells) == 0:
        return []
    with L.DensityPopulation.upload(layout, None) as pop:
        values = population_compartment_densities(pop, chr_2_AB_dict, gaussian_radius, normalize_by_reg_num=normalize_by_reg_num,
                                                  exclude_self=exclude_self, use_cis=use_cis, use_trans=use_trans)
    return layout.unpack(values)


def calculate_compartment_densities(chr_2_zxys, chr_2_AB_dict,
                                    gaussian_radius,
                                    normalize_by_reg_num=False,
                                    exclude_self=True,
                                    use_cis=False, use_trans=True,
                                    ):
    """Function to calculate comaprtment densities based on single-cell chr-2-zxys (:11-87): the batch of one cell."""
    return BatchCompartmentDensities([chr_2_zxys], chr_2_AB_dict, gaussian_radius, normalize_by_reg_num=normalize_by_reg_num,
                                     exclude_self=exclude_self, use_cis=use_cis, use_trans=use_trans)[0]
