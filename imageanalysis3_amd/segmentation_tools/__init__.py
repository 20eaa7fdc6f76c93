"""segmentation_tools — what the spot path needs of the reference's segmentation_tools: the bounding boxes of a label
image (cell.py), the candidate chromosomes of a whole stack (chromosome.py: find_candidate_chromosomes), their selection
by the candidate spots of every round (chromosome.py: select_candidate_chromosomes, on spot_tools.picking.
assign_spots_to_chromosomes) and the operators they are made of (morphology.py: 3-D binary erosion / dilation / closing by
ball(r), hole filling, 6-connected labelling, small-object removal, label centres), all on the device.  Cellpose, the
OpenCV warps, the watershed steps and the other chromosome finders (find_candidate_chromosomes_in_nucleus,
identify_chromosomes) stay the reference's."""
