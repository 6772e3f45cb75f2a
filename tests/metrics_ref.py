"""Float64 restatement of the four image metrics of etainv_image_metrics (include/etainv.h), and the seeded cases the metric tests share.

Everything from the normalisation on is float64; only the window is what the reference uses, its float32 values (exp and normalisation rounded
to float32), widened.  One pair at a time: `pred`, `target` are (3, H, W) float32 tensors in `input_range`."""
import math

import torch

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
NAMES = ("mse", "psnr", "ssim", "msssim")


def window64():
    c = torch.arange(11, dtype=torch.float32) - 5
    g = torch.exp(-(c ** 2) / (2 * 1.5 ** 2))
    return (g / g.sum()).double()


def normalise(x, input_range=(-1, 1)):
    lo, hi = input_range
    return (x.double() - lo) / (hi - lo)


def window_mean(x, win):
    """weighted mean under the 11-tap window at every position where it fits: along H, then along W.  x (C, H, W) float64"""
    rows = x.unfold(1, 11, 1)                                   # (C, H - 10, W, 11)
    x = (rows * win).sum(-1)
    cols = x.unfold(2, 11, 1)                                   # (C, H - 10, W - 10, 11)
    return (cols * win).sum(-1)


def moments(x, y, win):
    mu1, mu2 = window_mean(x, win), window_mean(y, win)
    return mu1, mu2, window_mean(x * x, win) - mu1 * mu1, window_mean(y * y, win) - mu2 * mu2, window_mean(x * y, win) - mu1 * mu2


def mse(pred, target, input_range=(-1, 1)):
    d = normalise(pred, input_range) - normalise(target, input_range)
    return (d * d).mean().item()


def psnr(pred, target, input_range=(-1, 1)):
    m = mse(pred, target, input_range)
    return math.inf if m == 0 else 10 * math.log10(1 / m)


def data_range(pred, target, input_range=(-1, 1)):
    x, y = normalise(pred, input_range), normalise(target, input_range)
    return max((x.max() - x.min()).item(), (y.max() - y.min()).item())


def ssim(pred, target, input_range=(-1, 1), data_range_override=None):
    """torchmetrics' StructuralSimilarityIndexMeasure() with its defaults: the range from the data (`data_range_override`: a given range instead).
    Range 0 (two constant images; torchmetrics divides 0 by 0): structure term 1, luminance term with C1 = 0, 0 / 0 = 1."""
    x, y = normalise(pred, input_range), normalise(target, input_range)
    r = data_range(pred, target, input_range) if data_range_override is None else data_range_override
    mu1, mu2, s11, s22, s12 = moments(x, y, window64())
    if r == 0:
        den = mu1 * mu1 + mu2 * mu2
        return torch.where(den > 0, 2 * mu1 * mu2 / den, torch.ones_like(den)).mean().item()
    c1, c2 = (0.01 * r) ** 2, (0.03 * r) ** 2
    return (((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s11 + s22 + c2))).mean().item()


def pool(x):
    """2 x 2 average pooling with `size % 2` rows / columns of zeros in front, which count in the divisor"""
    _, h, w = x.shape
    ph, pw = h % 2, w % 2
    padded = torch.zeros(x.shape[0], h + 2 * ph, w + 2 * pw, dtype=x.dtype)
    padded[:, ph:ph + h, pw:pw + w] = x
    hp, wp = (h + 2 * ph - 2) // 2 + 1, (w + 2 * pw - 2) // 2 + 1
    p = padded[:, :2 * hp, :2 * wp]
    return (p[:, 0::2, 0::2] + p[:, 0::2, 1::2] + p[:, 1::2, 0::2] + p[:, 1::2, 1::2]) / 4


def msssim(pred, target, input_range=(-1, 1)):
    x, y = normalise(pred, input_range), normalise(target, input_range)
    assert min(x.shape[1:]) > 160
    win, c1, c2 = window64(), 0.01 ** 2, 0.03 ** 2
    out = torch.ones(3, dtype=torch.float64)
    for level, weight in enumerate(WEIGHTS):
        mu1, mu2, s11, s22, s12 = moments(x, y, win)
        cs = (2 * s12 + c2) / (s11 + s22 + c2)
        if level < len(WEIGHTS) - 1:
            term = cs.mean(dim=(1, 2))
            x, y = pool(x), pool(y)
        else:
            term = ((2 * mu1 * mu2 + c1) / (mu1 * mu1 + mu2 * mu2 + c1) * cs).mean(dim=(1, 2))
        out = out * term.clamp(min=0) ** weight
    return out.mean().item()


def all_metrics(pred, target, input_range=(-1, 1)):
    h, w = pred.shape[1:]
    out = {"mse": mse(pred, target, input_range), "psnr": psnr(pred, target, input_range)}
    if min(h, w) >= 11:
        out["ssim"] = ssim(pred, target, input_range)
    if min(h, w) > 160:
        out["msssim"] = msssim(pred, target, input_range)
    return out


# ---- the seeded cases (tests/golden/make_metrics_golden.py records the reference's float32 values of the same pairs)
SMALL = [("11x11", 11, 11, 101), ("12x17", 12, 17, 102), ("11x40", 11, 40, 103), ("37x75", 37, 75, 104), ("64x64_narrow", 64, 64, 105)]
LARGE = [("161x161", 161, 161, 201), ("161x176", 161, 176, 202), ("168x165", 168, 165, 203), ("192x192", 192, 192, 204)]
CASES = SMALL + LARGE


def make_pair(name, h, w, seed):
    """(pred, target) (3, h, w) float32 in (-1, 1): uniform noise in [0, 1], the second image the first plus 0.1 randn, clamped; mapped to (-1, 1).
    `64x64_narrow`: both scaled into [0.4, 0.65] first, so that the range taken from the data is about 0.25"""
    g = torch.Generator().manual_seed(seed)
    a = torch.rand(3, h, w, generator=g)
    b = (a + 0.1 * torch.randn(3, h, w, generator=g)).clamp(0, 1)
    if name.endswith("narrow"):
        a, b = 0.4 + 0.25 * a, 0.4 + 0.25 * b
    return a * 2 - 1, b * 2 - 1


def degenerate_pairs(h=161, w=176, seed=301):
    """{name: (pred, target)}: identical images; two different constant images (zero variance); an anti-correlated pair (cs < 0 on the
    fine levels: the clamp at 0)"""
    g = torch.Generator().manual_seed(seed)
    a = torch.rand(3, h, w, generator=g) * 2 - 1
    return {"identical": (a, a.clone()),
            "constants": (torch.full((3, h, w), -0.25), torch.full((3, h, w), 0.5)),
            "anticorrelated": (a, -a)}
