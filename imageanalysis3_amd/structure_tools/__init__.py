"""structure_tools — what a tracing experiment is run for: the median distance map and the contact-probability map of a
population of picked chromosomes (distance.py: Chr2ZxysList_2_summaryDist_by_key, Chr2ZxysList_2_summaryDict, contact_prob
and the plotting-order helpers), summarised on the device without the stack of per-cell matrices, and the density clouds of
a traced nucleus (chromosome.py: convert_chr2Zxys_2_Cloud), rendered on the device.  contact.py and what builds on the maps
(the figures, and of domain_tools everything but its distance.py, which is in this package) stay the reference's; of
compartment_tools the A/B densities (density.py) are in this package,
its scoring.py and calling.py stay the reference's."""
from . import chromosome  # noqa: F401
