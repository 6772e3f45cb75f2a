"""The lpips and bglpips metrics (reference metrics/metrics.py:40-61, metrics/bglpips.py:15-150): `LPIPSMetric`, `BGLPIPS` and `lpips_distance`,
the batched call they sit on.

LPIPS v0.1 with net='alex', lpips=True, spatial=False in eval mode, restated (neither the lpips package nor torchvision is a dependency): the
images go from `input_range` to [-1, 1]; bglpips multiplies them by (1 - mask) there, so the foreground becomes 0; the scaling layer
(v - shift) / scale; torchvision's AlexNet `features`, tapped after each of its five ReLUs; per tap and pixel both feature vectors are divided
by (their norm + 1e-10), the squared difference is weighted by the tap's non-negative `lin` weights and summed over the channels, then averaged
over the tap's pixels; the score is the sum of the five means.  Lower is better.

Device tensors go to the HIP kernels (csrc/lpips.hip and NativeLpipsAlex of etainv/nets.py: one preprocess launch and one tower pass for the 2 B
images, five distance calls that add into one float64 [B]).  CPU tensors, or device="cpu", go to the plain-torch float32 path below
(F.conv2d / F.max_pool2d), which keeps the package and compute_metrics.py usable without a GPU.

Weights are handed over explicitly (`weights=`: a path, a pair of paths (backbone, linear heads), a state dict, a loaded `LpipsModel`, or
"synthetic"); there is no default and no download.  Not built: the reference's dump of every mask to result/mask/<i>/ (bglpips.py:115-124,
:94-95), which needs cv2 and serves debugging only."""
from typing import Optional, Tuple

import torch
import torch.nn.functional as F

from .base import SimpleMetric

MIN_SIDE = 31                          # the smallest input that leaves one pixel at tap 3


def _range(input_range) -> Tuple[float, float]:
    lo, hi = (0.0, 1.0) if input_range is None else (float(input_range[0]), float(input_range[1]))
    if not hi > lo:
        raise ValueError(f"input_range must be (lo, hi) with hi > lo, got {input_range}")
    return lo, hi


def _check_images(x: torch.Tensor) -> None:
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f"Input images should be (B, 3, H, W) tensors, but got {tuple(x.shape)}")
    if min(x.shape[2:]) < MIN_SIDE:
        raise ValueError(f"lpips takes images of at least {MIN_SIDE} x {MIN_SIDE} pixels (smaller ones leave no pixel at AlexNet's third tap), but got "
                         f"{tuple(x.shape[2:])}")


def _check_mask(mask: torch.Tensor, b: int, h: int, w: int) -> torch.Tensor:
    """-> float32 [1 or B][H][W], foreground = 1"""
    if mask.dtype != torch.float32:
        raise ValueError(f"the mask must be float32 (foreground = 1), got {mask.dtype}")
    if mask.dim() == 2:
        mask = mask[None]
    if mask.dim() != 3 or mask.shape[0] not in (1, b) or tuple(mask.shape[1:]) != (h, w):
        raise ValueError(f"the mask must be ({h}, {w}), (1, {h}, {w}) or ({b}, {h}, {w}) like the images, but got {tuple(mask.shape)}")
    return mask


class _TorchLpips:
    """the tower in plain float32 torch on the CPU, over the names of weights.lpips_shapes"""

    def __init__(self, sd: dict):
        from etainv.weights import LPIPS_CONVS, LPIPS_KERNELS
        self.convs = [(sd[f"features.{n}.weight"].float(), sd[f"features.{n}.bias"].float()) + LPIPS_KERNELS[i][1:] for i, n in enumerate(LPIPS_CONVS)]
        self.lins = [sd[f"lin{i}.model.1.weight"].float().reshape(-1) for i in range(5)]
        self.widths = tuple(w.shape[0] for w, *_ in self.convs)

    def __call__(self, x: torch.Tensor):
        """scaled images [n][3][H][W] -> the five taps [n][C][h][w]"""
        taps = []
        for i, (w, b, stride, pad) in enumerate(self.convs):
            if i in (1, 2):
                x = F.max_pool2d(x, 3, 2)
            x = F.relu(F.conv2d(x, w, b, stride=stride, padding=pad))
            taps.append(x)
        return taps


class LpipsModel:
    """A loaded LPIPS AlexNet for the metrics: the tower and the five `lin` heads on one device."""

    def __init__(self, weights, device: Optional[str] = None, net: str = "alex", compute_dtype=torch.float16, seed: int = 0):
        """`weights`: a path or state dict in the form of lpips.LPIPS(net='alex').state_dict(), torchvision's AlexNet names with the `lin` keys, a
        pair (backbone, linear heads), a loaded `LpipsModel` (shared as it is), or "synthetic" (then `net` picks the widths: "alex", or "tiny"
        for quick CPU runs)."""
        from etainv.weights import load_lpips_state_dict, synthetic_lpips_state_dict
        if isinstance(weights, LpipsModel):
            self.__dict__.update(weights.__dict__)
            return
        if weights is None:
            raise ValueError("lpips needs weights=: a path, a pair of paths, a state dict or \"synthetic\" (there is no default and no download)")
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        if net not in ("alex", "tiny"):
            raise NotImplementedError(f"lpips net '{net}' is not built: the reference uses net='alex' (metrics.py:56, bglpips.py:27)")
        self.device, self.net = str(device), net
        self.synthetic = isinstance(weights, str) and weights == "synthetic"
        sd = synthetic_lpips_state_dict(seed=seed, net=net) if self.synthetic else load_lpips_state_dict(weights)
        if self.device.startswith("cuda"):
            from etainv.nets import NativeLpipsAlex
            with torch.cuda.device(self.device):
                self.backend = NativeLpipsAlex(sd, compute_dtype=compute_dtype)
            self.dtype = compute_dtype
        else:
            self.backend, self.dtype = _TorchLpips(sd), torch.float32
        self.widths = tuple(self.backend.widths)


def lpips_preprocess(x: torch.Tensor, input_range=(-1, 1), mask: Optional[torch.Tensor] = None, dtype=torch.float16) -> torch.Tensor:
    """(n, 3, H, W) images in `input_range` -> what the tower reads.  Device tensors: one etainv_lpips_preprocess launch, [n][H][W][4] NHWC in
    `dtype` with a zero fourth channel; CPU tensors: float32 [n][3][H][W].  `mask` [n_mask][H][W] float32, foreground = 1: image i is multiplied
    by 1 - mask[i % n_mask] after the map to [-1, 1]."""
    from etainv.weights import LPIPS_SCALE, LPIPS_SHIFT
    lo, hi = _range(input_range)
    n, _, h, w = x.shape
    if not x.is_cuda:
        v = 2.0 * ((x.detach().float() - lo) / (hi - lo)) - 1.0
        if mask is not None:
            v = v * (1.0 - mask.float().repeat(n // mask.shape[0], 1, 1)[:, None])
        return (v - torch.tensor(LPIPS_SHIFT).view(1, 3, 1, 1)) / torch.tensor(LPIPS_SCALE).view(1, 3, 1, 1)
    from etainv import _capi
    lib = _capi.load()
    x = x.detach().to(torch.float32).contiguous()
    if mask is not None:
        mask = mask.to(device=x.device, dtype=torch.float32).contiguous()
    with torch.cuda.device(x.device):
        out = torch.empty(n, h, w, 4, dtype=dtype, device=x.device)
        _capi.check(lib.etainv_lpips_preprocess(_capi.ptr(x), _capi.ptr(mask), n, 0 if mask is None else mask.shape[0], h, w, lo, hi, _capi.ptr(out),
                                                _capi.dtype_code(dtype), _capi.stream_ptr()))
    return out


def layer_distance(feats: torch.Tensor, lin_w: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """feats [2 B][pixels][C] (rows 0 .. B-1 the sources', B .. 2B-1 the edits'), lin_w [C] -> float64 [B]: the mean over the pixels of
    sum_c lin_w[c] (a_c / (|a| + 1e-10) - b_c / (|b| + 1e-10))^2; with `out`, added to it.  Device tensors: one etainv_lpips_layer_distance
    call; CPU tensors: float64 torch."""
    if feats.dim() != 3 or feats.shape[0] % 2:
        raise ValueError(f"feats must be [2 B][pixels][C], got {tuple(feats.shape)}")
    b2, pixels, c = feats.shape
    if not feats.is_cuda:
        f = feats.double()
        f = f / (f.square().sum(-1, keepdim=True).sqrt() + 1e-10)
        d = ((f[:b2 // 2] - f[b2 // 2:]).square() * lin_w.double()).sum(-1).mean(-1)
        return d if out is None else out + d
    from etainv import _capi
    lib = _capi.load()
    feats = feats.contiguous()
    with torch.cuda.device(feats.device):
        need = lib.etainv_lpips_distance_workspace_bytes(b2 // 2, pixels)
        if need < 0:
            raise _capi.EtainvError(lib.etainv_last_error().decode())
        ws = torch.empty(need // 8 + 1, dtype=torch.float64, device=feats.device)
        acc = out is not None
        if not acc:
            out = torch.empty(b2 // 2, dtype=torch.float64, device=feats.device)
        _capi.check(lib.etainv_lpips_layer_distance(_capi.ptr(feats), _capi.ptr(lin_w), b2 // 2, pixels, c, int(acc), _capi.ptr(out), _capi.ptr(ws),
                                                    ws.numel() * 8, _capi.dtype_code(feats.dtype), _capi.stream_ptr()))
    return out


def lpips_taps(x: torch.Tensor, model: LpipsModel, input_range=(-1, 1), mask: Optional[torch.Tensor] = None):
    """(n, 3, H, W) -> the model's five taps, each [n][pixels][C] in the model's dtype on its device (valid until the next call of that shape)"""
    _check_images(x)
    x = x.to(model.device)
    if mask is not None:
        mask = mask.to(model.device)
    if x.is_cuda:
        with torch.cuda.device(x.device):
            return model.backend(lpips_preprocess(x, input_range, mask, model.dtype), x.shape[0])
    return [t.flatten(2).transpose(1, 2) for t in model.backend(lpips_preprocess(x, input_range, mask))]


def lpips_distance(edit: torch.Tensor, source: torch.Tensor, model: LpipsModel, input_range=(-1, 1), mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """float64 [B] LPIPS distances of B pairs: `edit` the edited images, `source` the input images, both (B, 3, H, W) in `input_range`, at least
    31 x 31.  `mask` ([B][H][W] or [H][W] float32, foreground = 1) gives bglpips: both images of pair i are multiplied by 1 - mask_i after the map
    to [-1, 1].  One preprocess launch and one tower pass for the 2 B images, five distance calls.  Every pair is independent: row i is what a
    call with pair i alone returns."""
    if edit.shape != source.shape:
        raise ValueError(f"Input images should have the same dimensions, but got {edit.shape} and {source.shape}.")
    _check_images(edit)
    if mask is not None:
        mask = _check_mask(mask, edit.shape[0], edit.shape[2], edit.shape[3])
    taps = lpips_taps(torch.cat([source.to(edit.device), edit]), model, input_range, mask)
    out = None
    for feats, lin_w in zip(taps, model.backend.lins):
        out = layer_distance(feats, lin_w, out)
    return out


class LPIPSMetric(SimpleMetric):
    """LPIPS metric.  Lower means better."""

    def __init__(self, input_range: Tuple[int, int] = (-1, 1), device: Optional[str] = None, weights=None, net: str = "alex") -> None:
        super().__init__(input_range, device)
        self.model = weights if isinstance(weights, LpipsModel) else LpipsModel(weights, self.device, net)

    def forward(self, pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        """one example: (1, 3, H, W) or (3, H, W) images in `input_range`; a batch gives (B, 1, 1, 1), as lpips.LPIPS does"""
        img = lambda t: t[None] if t.dim() == 3 else t
        rows = lpips_distance(img(target), img(pred), self.model, self.input_range)
        return rows.reshape(-1, 1, 1, 1)

    def __repr__(self) -> str:
        return "lpips"


class BGLPIPS(SimpleMetric):
    """BG-LPIPS metric.  Lower means better.  LPIPS on the background only (where no edit is wanted), by a foreground mask."""

    def __init__(self, input_range: Tuple[int, int] = (-1, 1), device: Optional[str] = None, weights=None, net: str = "alex") -> None:
        super().__init__(input_range, device)
        self.model = weights if isinstance(weights, LpipsModel) else LpipsModel(weights, self.device, net)

    def forward(self, source_image: torch.Tensor, target_image: torch.Tensor, prompt: str, mask: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
        """`mask`: float32 (H, W), (1, H, W) or (B, H, W), 1 = foreground; None: None is returned and nothing is recorded (`prompt` is unused)"""
        if mask is None:
            return None
        if not torch.is_tensor(mask):
            mask = torch.from_numpy(mask)
        img = lambda t: t[None] if t.dim() == 3 else t
        rows = lpips_distance(img(target_image), img(source_image), self.model, self.input_range, mask=mask)
        return rows.reshape(-1, 1, 1, 1)

    def __repr__(self) -> str:
        return "bglpips"
