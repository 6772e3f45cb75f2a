"""References for the lpips and bglpips metrics (torch only; the one import of the library is its synthetic weights): LPIPS v0.1 with net='alex',
lpips=True, spatial=False in eval mode, restated in float64 -- the range map, the background mask, the scaling layer, torchvision's AlexNet
`features` tapped after each ReLU, the channel normalisation with the epsilon added to the norm, the `lin` weights, the spatial mean and the sum
over the five taps.  The convolution is an explicit gather of every window followed by an einsum and the pooling a maximum over nine strided
slices, so that tests/test_lpips_ref.py, which pins them to F.conv2d / F.max_pool2d, compares two different computations.  `Prec(dtype)` (of
tests/dino_ref.py) gives the execution in a 16-bit or fp32 type: every operand and result rounded to the dtype, fp32 arithmetic between two
rounding points; the distance itself is float64 from the rounded features on, as the kernel's is."""
import torch

from tests.dino_ref import Prec

SHIFT, SCALE = (-.030, -.088, -.188), (.458, .448, .450)
CONVS = (0, 3, 6, 8, 10)                                  # positions in torchvision's `features`
KERNELS = ((11, 4, 2), (5, 1, 2), (3, 1, 1), (3, 1, 1), (3, 1, 1))       # (kernel, stride, pad)
EPS = 1e-10


def preprocess(x, lo, hi, mask=None, work=torch.float64):
    """[n][3][H][W] in (lo, hi) -> the scaled images in `work`; mask [n_mask][H][W], foreground = 1: image i is multiplied by 1 - mask[i % n_mask]
    after the map to [-1, 1] and before the scaling layer"""
    v = 2.0 * ((x.to(work) - lo) / (hi - lo)) - 1.0
    if mask is not None:
        idx = torch.arange(x.shape[0]) % mask.shape[0]
        v = v * (1.0 - mask.to(work)[idx][:, None])
    return (v - torch.tensor(SHIFT, dtype=work).view(1, 3, 1, 1)) / torch.tensor(SCALE, dtype=work).view(1, 3, 1, 1)


def out_size(s, k, stride, pad):
    return (s + 2 * pad - k) // stride + 1


def pool_size(s):
    return (s - 3) // 2 + 1


def tap_sizes(h, w):
    t1 = (out_size(h, 11, 4, 2), out_size(w, 11, 4, 2))
    t2 = (pool_size(t1[0]), pool_size(t1[1]))
    t3 = (pool_size(t2[0]), pool_size(t2[1]))
    return [t1, t2, t3, t3, t3]


def conv2d(x, w, b, stride, pad):
    """[n][C][H][W] * [O][C][kh][kw] -> [n][O][Ho][Wo]: every window gathered from the zero-padded image, then one einsum"""
    n, c, h, wd = x.shape
    o, _, kh, kw = w.shape
    xp = torch.zeros(n, c, h + 2 * pad, wd + 2 * pad, dtype=x.dtype)
    xp[:, :, pad:pad + h, pad:pad + wd] = x
    ho, wo = out_size(h, kh, stride, pad), out_size(wd, kw, stride, pad)
    iy = torch.arange(ho)[:, None] * stride + torch.arange(kh)[None, :]
    ix = torch.arange(wo)[:, None] * stride + torch.arange(kw)[None, :]
    win = xp[:, :, iy[:, None, :, None], ix[None, :, None, :]]               # [n][C][Ho][Wo][kh][kw]
    return torch.einsum("nchwyx,ocyx->nohw", win, w.to(x.dtype)) + b.to(x.dtype).view(1, -1, 1, 1)


def maxpool3s2(x):
    """window 3, stride 2, floor mode, no padding: the maximum over nine strided slices"""
    ho, wo = pool_size(x.shape[-2]), pool_size(x.shape[-1])
    out = None
    for dy in range(3):
        for dx in range(3):
            s = x[..., dy:dy + 2 * ho - 1:2, dx:dx + 2 * wo - 1:2]
            out = s if out is None else torch.maximum(out, s)
    return out


def taps(sd, v, pr=Prec()):
    """scaled images [n][3][H][W] -> the five taps [n][C][h][w] in pr.work; with a dtype, the stored points (the scaled image, the weights, every
    conv + ReLU result) are rounded to it"""
    x = pr.r(v.to(pr.work), "embed")
    out = []
    for i, n in enumerate(CONVS):
        _, stride, pad = KERNELS[i]
        if i in (1, 2):
            x = maxpool3s2(x)
        y = conv2d(x, pr.r(sd[f"features.{n}.weight"].to(pr.work), "weight"), sd[f"features.{n}.bias"], stride, pad)
        x = pr.r(torch.clamp(y, min=0), "gemm_out")
        out.append(x)
    return out


def tap_distance(f0, f1, w):
    """[B][C][h][w] features of both sides, lin weights [C] -> float64 [B]"""
    f0, f1 = f0.double(), f1.double()
    n0 = f0 / (f0.square().sum(1, keepdim=True).sqrt() + EPS)
    n1 = f1 / (f1.square().sum(1, keepdim=True).sqrt() + EPS)
    return ((n0 - n1).square() * w.double().view(1, -1, 1, 1)).sum(1).mean((-1, -2))


def lins(sd):
    return [sd[f"lin{i}.model.1.weight"].reshape(-1) for i in range(5)]


def score(sd, x, b, lo, hi, mask=None, pr=Prec()):
    """images [2 b][3][H][W] (sources, then edits) -> (float64 [b] scores, the five taps as float64)"""
    t = [f.double() for f in taps(sd, preprocess(x, lo, hi, mask, pr.work), pr)]
    s = torch.zeros(b, dtype=torch.float64)
    for f, w in zip(t, lins(sd)):
        s = s + tap_distance(f[:b], f[b:], w)
    return s, t


# ---------------------------------------------------------------------------------------------------------------- inputs
def make_images(b, h, w, seed, noise=0.1):
    """(source, edit), each (b, 3, h, w) float32 inside [-1, 1]: smooth structure plus noise.  Even pairs: the edit is the source plus `noise`
    N(0, 1) (a reconstruction); odd pairs: an independent image"""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, h), torch.linspace(0, 1, w), indexing="ij")

    def draw():
        phase = torch.rand(b, 3, 1, 1, generator=g) * 6.28
        return 0.5 * torch.sin(9 * xx + phase) * torch.cos(7 * yy - phase) + 0.25 * torch.randn(b, 3, h, w, generator=g)

    src, other = draw(), draw()
    recon = src + noise * torch.randn(b, 3, h, w, generator=g)
    even = (torch.arange(b) % 2 == 0).view(b, 1, 1, 1)
    return src.clamp(-1, 1).float(), torch.where(even, recon, other).clamp(-1, 1).float()


def make_masks(b, h, w, seed):
    """float32 [b][h][w], foreground = 1: one rectangle per pair, between a sixth and a half of each side"""
    g = torch.Generator().manual_seed(seed)
    m = torch.zeros(b, h, w)
    for i in range(b):
        hh, ww = int(h * (0.17 + 0.33 * torch.rand(1, generator=g))), int(w * (0.17 + 0.33 * torch.rand(1, generator=g)))
        y0, x0 = int(torch.randint(0, h - hh, (1,), generator=g)), int(torch.randint(0, w - ww, (1,), generator=g))
        m[i, y0:y0 + hh, x0:x0 + ww] = 1.0
    return m


# (tests/golden/make_lpips_golden.py records the float64 scores, a subset of the tap values and the yardsticks in tests/golden/lpips_ref.npz;
# models and images are drawn from these seeds, not stored)
CASES = {"s64": dict(pairs=4, h=64, w=64, seed=301, mask=False), "s67": dict(pairs=4, h=67, w=70, seed=302, mask=False),
         "m64": dict(pairs=4, h=64, w=64, seed=301, mask=True), "m67": dict(pairs=4, h=67, w=70, seed=302, mask=True),
         "big": dict(pairs=1, h=512, w=512, seed=303, mask=False)}
SMALL = ("s64", "s67", "m64", "m67")
TAP_STRIDE = 23                                           # the fixture keeps every 23rd value of every tap of the small cases
MODEL_SEED = 0


def model_state_dict(net="alex"):
    """the library's synthetic LPIPS weights (the one import of the library here)"""
    from etainv.weights import synthetic_lpips_state_dict
    return synthetic_lpips_state_dict(seed=MODEL_SEED, net=net)


def case_inputs(case):
    """(images [2 pairs][3][h][w] = sources then edits in (-1, 1), pairs, mask [pairs][h][w] or None)"""
    c = CASES[case]
    src, edit = make_images(c["pairs"], c["h"], c["w"], c["seed"])
    return torch.cat([src, edit]), c["pairs"], make_masks(c["pairs"], c["h"], c["w"], c["seed"] + 50) if c["mask"] else None
