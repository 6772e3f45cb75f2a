"""Metric base classes (reference metrics/base.py:6-102): a metric is called on one example, `update` records its value, `compute` averages the
recorded values and forgets them."""
from typing import Dict, List, Optional, Tuple, Union

import numpy as np
import torch


class BaseMetric:
    def __init__(self, input_range: Optional[Tuple[int, int]] = (-1, 1), device: Optional[str] = None) -> None:
        """`input_range`: the value range of the image tensors (None: already [0, 1]); `device`: where the metric is computed (None: "cuda" when
        there is one, else "cpu")"""
        self.input_range = input_range
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        self.device = device

    def _normalize(self, x: torch.Tensor) -> torch.Tensor:
        """`x` mapped from `input_range` to [0, 1]"""
        if self.input_range is None:
            return x
        return (x - self.input_range[0]) / (self.input_range[1] - self.input_range[0])

    def __call__(self, *args, **kwargs) -> Union[torch.Tensor, None]:
        return self.forward(*args, **kwargs)

    def forward(self, *args, **kwargs) -> Union[torch.Tensor, None]:
        """the metric of one example (None: it could not be computed)"""
        raise NotImplementedError

    def update(self, *args, **kwargs) -> Union[float, None]:
        """compute the metric of one example, record it and return it"""
        raise NotImplementedError

    def compute(self) -> Tuple[float, Dict[str, Union[float, List[float]]]]:
        """(mean, {"value": mean, "all": recorded values}) over the examples recorded since the last call"""
        raise NotImplementedError


class SimpleMetric(BaseMetric):
    def __init__(self, input_range: Optional[Tuple[int, int]] = (-1, 1), device: Optional[str] = None) -> None:
        super().__init__(input_range=input_range, device=device)
        self.losses = []

    def update(self, *args, **kwargs) -> Union[float, None]:
        loss = self.forward(*args, **kwargs)
        if loss is None:
            return None
        self.losses.append(loss.detach().cpu().numpy().item())
        return self.losses[-1]

    def compute(self) -> Tuple[float, Dict[str, Union[float, List[float]]]]:
        mean = np.mean(self.losses).astype(float).item()
        out = mean, {"value": mean, "all": self.losses}
        self.losses = []
        return out


class KernelMetric(SimpleMetric):
    """One of the four metrics of `image_metrics`.  The normalisation of `_normalize` happens inside that call (on the device: inside the kernels),
    the inputs are moved to the metric's device, and a batch of more than one pair gives the mean of its rows."""
    name = None

    def forward(self, pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        from .functional import image_metrics
        rows = image_metrics(pred.to(self.device), target.to(self.device), self.input_range, (self.name,))[self.name]
        return rows[0] if rows.shape[0] == 1 else rows.mean()

    def __repr__(self) -> str:
        return self.name
