"""Image metrics of saved edits (reference metrics/): `EditMetric` over the metric classes, and `image_metrics` / `clip_scores` / `dino_structure` /
`lpips_distance`, the batched calls they sit on."""
from .base import BaseMetric, SimpleMetric
from .clip_similarity import CLIPAccuracy, CLIPSimilarity, ClipModel, clip_scores
from .dino_vit_structure import Dinov2Model, DinoModel, DinoVitStructure, dino_structure
from .edit_metric import EditMetric
from .functional import NAMES, image_metrics
from .lpips import BGLPIPS, LPIPSMetric, LpipsModel, lpips_distance
from .metrics import MSEMetric, PSNRMetric
from .msssim import MSSSIM
from .ssim import SSIM

__all__ = ["BaseMetric", "SimpleMetric", "EditMetric", "MSEMetric", "PSNRMetric", "SSIM", "MSSSIM", "image_metrics", "NAMES", "CLIPSimilarity", "CLIPAccuracy",
           "ClipModel", "clip_scores", "DinoVitStructure", "DinoModel", "Dinov2Model", "dino_structure", "LPIPSMetric", "BGLPIPS", "LpipsModel", "lpips_distance"]
