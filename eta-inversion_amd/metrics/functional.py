"""`image_metrics`: MSE, PSNR, SSIM and MS-SSIM of B image pairs in one call -- the batched function the metric classes sit on.

Device tensors go to the fused HIP kernels (etainv_image_metrics, csrc/metrics.hip: float64 arithmetic, fixed summation order).  CPU tensors go to
the plain-torch float32 path below, which keeps the package and compute_metrics.py usable without a GPU; it runs the operations of the
reference's classes in their order (metrics/metrics.py:7-34, metrics/msssim.py:61-106, :168-247) pair by pair, so a row equals the reference's
B = 1 call.  `ssim` is torchmetrics.image.StructuralSimilarityIndexMeasure() with its defaults [3P] (metrics/ssim.py:15), restated: the
11-tap sigma-1.5 window, k1 = 0.01, k2 = 0.03, reflect padding by 5 cropped by 5 again (= the unpadded window), the mean over all channels and
window positions, and data_range=None, i.e. the range max(pred.max() - pred.min(), target.max() - target.min()) of the normalised pair."""
from typing import Dict, Optional, Sequence, Tuple, Union

import torch
import torch.nn.functional as F

NAMES = ("mse", "psnr", "ssim", "msssim")
_BIT = {"mse": 1, "psnr": 2, "ssim": 4, "msssim": 8}
WIN_SIZE = 11
MSSSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
MSSSIM_MIN_SIDE = (WIN_SIZE - 1) * 2 ** 4          # the smaller side must exceed it
# the float32 window the reference builds (metrics/msssim.py:15-29: exp(-(i - 5)^2 / (2 * 1.5^2)) and its normalisation rounded to float32);
# csrc/metrics.hip holds the same constants, tests/test_metrics_host.py pins both to what torch computes
WINDOW_HEX = ("0x1.0d957p-10", "0x1.f1fe02p-8", "0x1.26eb18p-5", "0x1.bff0fep-4", "0x1.b43c3ep-3", "0x1.10656p-2",
              "0x1.b43c3ep-3", "0x1.bff0fep-4", "0x1.26eb18p-5", "0x1.f1fe02p-8", "0x1.0d957p-10")


def gaussian_window(dtype=torch.float32) -> torch.Tensor:
    return torch.tensor([float.fromhex(h) for h in WINDOW_HEX], dtype=dtype)


def _blur(x: torch.Tensor, win: torch.Tensor) -> torch.Tensor:
    """the window along H, then along W, no padding; one filter per channel"""
    c = x.shape[1]
    x = F.conv2d(x, win.view(1, 1, -1, 1).repeat(c, 1, 1, 1), groups=c)
    return F.conv2d(x, win.view(1, 1, 1, -1).repeat(c, 1, 1, 1), groups=c)


def _ssim_cs(x: torch.Tensor, y: torch.Tensor, data_range, win: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """per (pair, channel) means of the ssim map and of the cs map"""
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    mu1, mu2 = _blur(x, win), _blur(y, win)
    mu11, mu22, mu12 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s11, s22, s12 = _blur(x * x, win) - mu11, _blur(y * y, win) - mu22, _blur(x * y, win) - mu12
    cs = (2 * s12 + c2) / (s11 + s22 + c2)
    ssim = ((2 * mu12 + c1) / (mu11 + mu22 + c1)) * cs
    return ssim.flatten(2).mean(-1), cs.flatten(2).mean(-1)


def _ssim_torch(x: torch.Tensor, y: torch.Tensor, win: torch.Tensor) -> torch.Tensor:
    data_range = torch.max(x.max() - x.min(), y.max() - y.min())
    if data_range == 0:
        # two constant images: both constants are 0 and torchmetrics divides 0 by 0.  Defined here as in the kernel: structure term 1 (its value
        # at zero variance for every C2 > 0), luminance term with C1 = 0, and 0 / 0 (both images 0) is 1
        mu1, mu2 = _blur(x, win), _blur(y, win)
        den = mu1.pow(2) + mu2.pow(2)
        return torch.where(den > 0, 2 * mu1 * mu2 / den, torch.ones_like(den)).mean()
    return _ssim_cs(x, y, data_range, win)[0].mean()


def _msssim_torch(x: torch.Tensor, y: torch.Tensor, win: torch.Tensor) -> torch.Tensor:
    weights = x.new_tensor(MSSSIM_WEIGHTS)
    terms = []
    for level in range(len(MSSSIM_WEIGHTS)):
        ssim, cs = _ssim_cs(x, y, 1.0, win)
        if level < len(MSSSIM_WEIGHTS) - 1:
            terms.append(torch.relu(cs))
            pad = [s % 2 for s in x.shape[2:]]                  # the padded zeros count in the divisor (count_include_pad)
            x, y = F.avg_pool2d(x, kernel_size=2, padding=pad), F.avg_pool2d(y, kernel_size=2, padding=pad)
    terms.append(torch.relu(ssim))
    stacked = torch.stack(terms, dim=0)                          # (level, pair, channel)
    return torch.prod(stacked ** weights.view(-1, 1, 1), dim=0).mean()


def _metrics_torch(pred: torch.Tensor, target: torch.Tensor, lo: float, hi: float, which: Sequence[str]) -> Dict[str, torch.Tensor]:
    win = gaussian_window()
    rows = {name: [] for name in which}
    for i in range(pred.shape[0]):
        x, y = (pred[i:i + 1] - lo) / (hi - lo), (target[i:i + 1] - lo) / (hi - lo)
        if "mse" in rows or "psnr" in rows:
            mse = F.mse_loss(x, y)
            if "mse" in rows:
                rows["mse"].append(mse)
            if "psnr" in rows:
                rows["psnr"].append(10 * torch.log10(1 / mse))
        if "ssim" in rows:
            rows["ssim"].append(_ssim_torch(x, y, win))
        if "msssim" in rows:
            rows["msssim"].append(_msssim_torch(x, y, win))
    return {name: torch.stack(v) if v else pred.new_zeros(0) for name, v in rows.items()}


def _metrics_device(pred: torch.Tensor, target: torch.Tensor, lo: float, hi: float, which: Sequence[str]) -> Dict[str, torch.Tensor]:
    from etainv import _capi
    lib = _capi.load()
    b, _, h, w = pred.shape
    mask = sum(_BIT[name] for name in set(which))
    with torch.cuda.device(pred.device):
        nbytes = lib.etainv_image_metrics_workspace_bytes(b, h, w, mask)
        if nbytes < 0:
            raise _capi.EtainvError(lib.etainv_last_error().decode())
        workspace = torch.empty(nbytes // 8, dtype=torch.float64, device=pred.device)
        out = torch.empty(b, 4, dtype=torch.float32, device=pred.device)
        _capi.check(lib.etainv_image_metrics(_capi.ptr(pred), _capi.ptr(target), b, h, w, float(lo), float(hi), mask, _capi.ptr(out),
                                             _capi.ptr(workspace), nbytes, _capi.stream_ptr()))
    return {name: out[:, NAMES.index(name)] for name in which}


def image_metrics(pred: torch.Tensor, target: torch.Tensor, input_range: Optional[Tuple[float, float]] = (-1, 1),
                  which: Union[str, Sequence[str]] = NAMES) -> Dict[str, torch.Tensor]:
    """{name: float32 tensor [B]} for the metrics named in `which`, of `pred` against `target`, both (B, 3, H, W) in `input_range` (None: already
    in [0, 1]).  Every pair is independent: row i is what a call with pair i alone returns.  `target` is moved to the device of `pred`;
    inputs that are not contiguous float32 are converted."""
    which = (which,) if isinstance(which, str) else tuple(which)
    unknown = [name for name in which if name not in NAMES]
    if unknown or not which:
        raise ValueError(f"image_metrics computes {', '.join(NAMES)}; got {list(which)}")
    if pred.shape != target.shape:
        raise ValueError(f"Input images should have the same dimensions, but got {pred.shape} and {target.shape}.")
    if pred.dim() != 4 or pred.shape[1] != 3:
        raise ValueError(f"Input images should be (B, 3, H, W) tensors, but got {pred.shape}")
    h, w = pred.shape[2:]
    if "ssim" in which and min(h, w) < WIN_SIZE:
        raise ValueError(f"ssim needs images of at least {WIN_SIZE} x {WIN_SIZE} pixels (one {WIN_SIZE}-tap window), but got {h} x {w}")
    if "msssim" in which and not min(h, w) > MSSSIM_MIN_SIDE:
        raise AssertionError("Image size should be larger than %d due to the 4 downsamplings in ms-ssim" % MSSSIM_MIN_SIDE)
    lo, hi = (0.0, 1.0) if input_range is None else (float(input_range[0]), float(input_range[1]))
    if not hi > lo:
        raise ValueError(f"input_range must be (lo, hi) with hi > lo, got {input_range}")
    pred = pred.detach().to(torch.float32).contiguous()
    target = target.detach().to(device=pred.device, dtype=torch.float32).contiguous()
    if pred.is_cuda:
        return _metrics_device(pred, target, lo, hi, which)
    return _metrics_torch(pred, target, lo, hi, which)
