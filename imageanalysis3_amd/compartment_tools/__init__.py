"""compartment_tools — the A/B compartment densities of traced cells (density.py: calculate_gaussian_density,
calculate_compartment_densities, BatchCompartmentDensities) as all-pairs sums on the device.  scoring.py and calling.py are
not here: importing them raises ImportError."""
from . import density  # noqa: F401
