"""SSIM (reference metrics/ssim.py:8-33: torchmetrics' StructuralSimilarityIndexMeasure with its defaults [3P], restated in functional.py)."""
from .base import KernelMetric


class SSIM(KernelMetric):
    "Structural Similarity Index Measure (SSIM) metric. Ranges from 1 (best) to 0 (worst)."
    name = "ssim"
