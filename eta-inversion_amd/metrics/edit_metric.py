"""One interface over the editing metrics (reference metrics/edit_metric.py:16-122).  Built: the four that need no pretrained network.  The CLIP,
DINO-ViT and LPIPS families stay listed and are refused by name."""
from typing import Dict, List, Optional, Tuple, Union

import numpy as np
import torch

from .base import SimpleMetric
from .metrics import MSEMetric, PSNRMetric
from .msssim import MSSSIM
from .ssim import SSIM

_BUILT = {"ssim": SSIM, "msssim": MSSSIM, "mse": MSEMetric, "psnr": PSNRMetric}
_NAMES = ["clip_text_img", "clip_img_img", "clip_text_text", "clip_textdir_imgdir", "clip_text_img_acc", "clip_text_text_acc", "dinovitstruct",
          "dinovitstruct_v2", "lpips", "bglpips", "ssim", "msssim", "mse", "psnr"]


class EditMetric(SimpleMetric):
    def __init__(self, name: str, input_range: Tuple[int, int] = (-1, 1), device: Optional[str] = None, **kwargs) -> None:
        """`name`: one of get_available_metrics()"""
        super().__init__(input_range, device)
        self.metric_name = name
        if name not in _BUILT:
            raise NotImplementedError(f"metric '{name}' is not built: built are {', '.join(_BUILT)}; the others ({', '.join(n for n in _NAMES if n not in _BUILT)}, "
                                      f"nslpips) need pretrained CLIP / DINO / LPIPS weights")
        self.metric = _BUILT[name](input_range=input_range, device=device, **kwargs)

    @staticmethod
    def get_available_metrics() -> List[str]:
        """the reference's metric names in its order (the built ones: see __init__)"""
        return list(_NAMES)

    @staticmethod
    def get_built_metrics() -> List[str]:
        return [n for n in _NAMES if n in _BUILT]

    def update(self, source_image: torch.Tensor, edit_image: torch.Tensor, source_prompt: str, target_prompt: str, edit_word: str,
               mask: Optional[torch.Tensor] = None) -> float:
        """record one example: `source_image` the input image, `edit_image` the edited output.  The four built metrics take
        (edit_image, source_image); prompts, edit word and mask are what the unbuilt ones take."""
        loss = self.metric.update(edit_image, source_image)
        if isinstance(loss, torch.Tensor):
            loss = loss.item()
        elif isinstance(loss, np.ndarray):
            loss = loss.astype(float).item()
        assert loss is None or isinstance(loss, float), f"{type(loss)}"
        return loss

    def compute(self) -> Tuple[float, Dict[str, Union[float, List[float]]]]:
        return self.metric.compute()

    def __repr__(self) -> str:
        return self.metric.__repr__()
