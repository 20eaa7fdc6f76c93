"""segmentation_tools — what the spot path needs of the reference's segmentation_tools: the bounding boxes of a label
image (cell.py).  Cellpose, the OpenCV warps and the watershed steps stay the reference's."""
