"""domain_tools — the distances under the reference's domain analysis (distance.py: _sliding_window_dist, domain_distance,
domain_pdists, domain_neighboring_dists, _domain_contact_freq) as three kernels on a resident population of traced
chromosomes.  calling.py, interaction.py and manual.py are not here: importing them raises ImportError."""
from . import distance  # noqa: F401
