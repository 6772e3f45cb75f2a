"""One interface over the editing metrics (reference metrics/edit_metric.py:16-122).  Built: the four that need no pretrained network, -- only
when weights are handed over with `clip_weights=` -- the four CLIP metrics that need no captioner, -- only with `dino_weights=` -- dinovitstruct, -- only with `dinov2_weights=` -- dinovitstruct_v2, and -- only with `lpips_weights=` -- lpips and bglpips.
Everything else stays listed and is refused by name."""
from typing import Dict, List, Optional, Tuple, Union

import numpy as np
import torch

from .base import SimpleMetric
from .metrics import MSEMetric, PSNRMetric
from .msssim import MSSSIM
from .ssim import SSIM

_BUILT = {"ssim": SSIM, "msssim": MSSSIM, "mse": MSEMetric, "psnr": PSNRMetric}
# built when `clip_weights=` is given: name -> (class name in .clip_similarity, its `metric`)
_CLIP = {"clip_text_img": ("CLIPSimilarity", "text_img"), "clip_img_img": ("CLIPSimilarity", "img_img"),
         "clip_textdir_imgdir": ("CLIPSimilarity", "textdir_imgdir"), "clip_text_img_acc": ("CLIPAccuracy", "text_img")}
_CLIP_BLIP = ("clip_text_text", "clip_text_text_acc")
_NAMES = ["clip_text_img", "clip_img_img", "clip_text_text", "clip_textdir_imgdir", "clip_text_img_acc", "clip_text_text_acc", "dinovitstruct",
          "dinovitstruct_v2", "lpips", "bglpips", "ssim", "msssim", "mse", "psnr"]


class EditMetric(SimpleMetric):
    def __init__(self, name: str, input_range: Tuple[int, int] = (-1, 1), device: Optional[str] = None, **kwargs) -> None:
        """`name`: one of get_available_metrics().  `clip_weights` (a path, a state dict, a loaded `ClipModel` or "synthetic"): builds the CLIP
        metrics; `clip_templates`, `clip_model`: their caption templates and, for synthetic weights, the geometry.  `dino_weights` (a path, a state
        dict, a loaded `DinoModel` or "synthetic"): builds dinovitstruct; `dino_model`: its printed name and, for synthetic weights, the geometry.
        `dinov2_weights` (a path, a state dict, a loaded `Dinov2Model` or "synthetic"): builds dinovitstruct_v2; `dinov2_model`: its printed name
        and, for synthetic weights, the geometry.
        `lpips_weights` (a path, a pair of paths, a state dict, a loaded `LpipsModel` or "synthetic"): builds lpips and bglpips; `lpips_net`:
        "alex" (or "tiny" with synthetic weights)."""
        super().__init__(input_range, device)
        self.metric_name = name
        clip_weights = kwargs.pop("clip_weights", None)
        clip_templates, clip_model = kwargs.pop("clip_templates", None), kwargs.pop("clip_model", "ViT-B/16")
        dino_weights, dino_model = kwargs.pop("dino_weights", None), kwargs.pop("dino_model", "dino_vitb8")
        dinov2_weights, dinov2_model = kwargs.pop("dinov2_weights", None), kwargs.pop("dinov2_model", "dinov2_vitb14")
        lpips_weights, lpips_net = kwargs.pop("lpips_weights", None), kwargs.pop("lpips_net", "alex")
        self.is_clip = clip_weights is not None and name in _CLIP
        if lpips_weights is not None and name == "nslpips":
            raise NotImplementedError("metric 'nslpips' is not built: besides the LPIPS weights it needs a whole inversion of every sample under an "
                                      "attention store for its mask (the reference leaves it out of its own list, edit_metric.py:67)")
        if lpips_weights is not None and name in ("lpips", "bglpips"):
            from .lpips import BGLPIPS, LPIPSMetric
            self.metric = (LPIPSMetric if name == "lpips" else BGLPIPS)(input_range=input_range, device=device, weights=lpips_weights, net=lpips_net, **kwargs)
            return
        if dinov2_weights is not None and name == "dinovitstruct_v2":
            from .dino_vit_structure import DinoVitStructure, Dinov2Model
            model = dinov2_weights if isinstance(dinov2_weights, Dinov2Model) else Dinov2Model(dinov2_weights, self.device, dinov2_model,
                                                                                                antialias=kwargs.pop("antialias", True))
            kwargs.pop("antialias", None)
            self.metric = DinoVitStructure(input_range=input_range, device=device, vit_model=dinov2_model, weights=model, **kwargs)
            return
        if dino_weights is not None and name == "dinovitstruct_v2":
            raise NotImplementedError("metric 'dinovitstruct_v2' is not built from dino_weights=: besides DINOv2 weights it needs a ViT with patch 14, "
                                      "LayerScale and interpolated position embeddings (reference metrics/dino_vit_structure.py:33-34, :121-122), "
                                      "which Dinov2Model is: pass dinov2_weights=")
        if dino_weights is not None and name == "dinovitstruct":
            from .dino_vit_structure import DinoVitStructure
            self.metric = DinoVitStructure(input_range=input_range, device=device, vit_model=dino_model, weights=dino_weights, **kwargs)
            return
        if clip_weights is not None and name in _CLIP_BLIP:
            raise NotImplementedError(f"metric '{name}' is not built: it needs a BLIP captioner (reference metrics/clip_similarity.py:128-157) besides "
                                      f"the CLIP weights")
        if self.is_clip:
            from . import clip_similarity
            cls, metric = _CLIP[name]
            own = {} if isinstance(clip_weights, clip_similarity.ClipModel) else {"templates": clip_templates}
            self.metric = getattr(clip_similarity, cls)(input_range=input_range, device=device, metric=metric, clip_model=clip_model,
                                                        use_imagenet_templates=own.get("templates") is not None, weights=clip_weights, **own, **kwargs)
            return
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
        (edit_image, source_image), the CLIP metrics the images and the prompts, dinovitstruct, dinovitstruct_v2 and lpips (source_image, edit_image), bglpips
        (source_image, edit_image, source_prompt, mask) as the reference does (edit_metric.py:93-97); the edit word is what the unbuilt ones take."""
        if self.is_clip:                                         # by keyword, reference edit_metric.py:102-105
            loss = self.metric.update(source_image=source_image, target_image=edit_image, source_prompt=source_prompt, target_prompt=target_prompt)
        elif self.metric_name in ("dinovitstruct", "dinovitstruct_v2", "lpips"):
            loss = self.metric.update(source_image, edit_image)
        elif self.metric_name == "bglpips":
            loss = self.metric.update(source_image, edit_image, source_prompt, mask)
        else:
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
