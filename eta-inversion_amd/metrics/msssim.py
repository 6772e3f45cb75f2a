"""MS-SSIM with data_range 1 (reference metrics/msssim.py:336-361 on :61-106, :168-247)."""
from .base import KernelMetric


class MSSSIM(KernelMetric):
    "Multi-Scale Structural Similarity (MS-SSIM). Ranges from 1 (best) to 0 (worst)."
    name = "msssim"
