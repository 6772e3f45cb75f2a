"""MSE and PSNR of normalised images (reference metrics/metrics.py:7-37).  The reference's LPIPSMetric needs pretrained weights: EditMetric."""
from .base import KernelMetric


class MSEMetric(KernelMetric):
    """mean squared difference over all elements of the pair"""
    name = "mse"


class PSNRMetric(KernelMetric):
    """10 log10(1 / mse); inf for identical images"""
    name = "psnr"
