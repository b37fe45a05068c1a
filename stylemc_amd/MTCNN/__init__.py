"""MTCNN face detector (drop-in for the reference's ``MTCNN`` package): host logic in numpy / PIL, the three nets on the
gfx950 kernels (stylemc_amd.mtcnn_hip)."""
from .detector import detect_faces  # noqa: F401
