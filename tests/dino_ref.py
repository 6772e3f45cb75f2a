"""References for the dinovitstruct metric (torch and numpy only; no import of the library, none of transformers): torch's antialiased bilinear
resize restated as tables, DINO's image preprocessing, a float64 DINO ViT tower over DINO's checkpoint names with the rounding points of a 16-bit
execution, the keys of the last block, their cosine self-similarity and the score, a tiny random model and input builders.
tests/test_dino_ref.py pins these helpers on the CPU (against F.interpolate, transformers' ViTModel and values recorded from the reference's own
code); the GPU tests use them."""
import math

import numpy as np
import torch

MEAN = (0.485, 0.456, 0.406)          # ImageNet normalisation
STD = (0.229, 0.224, 0.225)
EPS = 1e-8                            # attn_cosine_sim's clamp on the product of the norms
LN_EPS = 1e-6


# ---------------------------------------------------------------------------------------------------------------- the resize
def resize_tables(n_in, n_out, antialias=True):
    """(bounds [n_out][2] = (first tap, taps) int32, coef [n_out][ksize] float64, rows sum to 1): the separable weights of
    F.interpolate(mode="bilinear", align_corners=False) along one axis.  antialias=True: a triangle of half-width max(scale, 1) around
    scale (i + 0.5), cut at the image's edges and renormalised; antialias=False: the two neighbours of scale (i + 0.5) - 0.5, clamped at 0.
    Trailing taps of weight zero are dropped (n_in == n_out: one tap of weight 1)."""
    scale = n_in / n_out
    rows = []
    for i in range(n_out):
        if antialias:
            support = max(scale, 1.0)
            c = scale * (i + 0.5)
            xmin = max(0, int(c - support + 0.5))
            xsize = min(n_in, int(c + support + 0.5)) - xmin
            w = [max(0.0, 1.0 - abs((j + xmin - c + 0.5) / support)) for j in range(xsize)]
            total = 0.0
            for v in w:
                total += v
            w = [v / total for v in w]
        else:
            src = max(scale * (i + 0.5) - 0.5, 0.0)
            xmin = min(int(src), n_in - 1)
            lam = src - xmin
            w = [1.0 - lam, lam] if xmin + 1 < n_in else [1.0]
        while len(w) > 1 and w[-1] == 0.0:
            w.pop()
        rows.append((xmin, w))
    ksize = max(len(w) for _, w in rows)
    bounds = np.zeros((n_out, 2), dtype=np.int32)
    coef = np.zeros((n_out, ksize), dtype=np.float64)
    for i, (xmin, w) in enumerate(rows):
        bounds[i] = (xmin, len(w))
        coef[i, :len(w)] = w
    return bounds, coef


def _pass(img, bounds, coef):
    """one resampling pass along the last axis, in the image's dtype"""
    out = torch.zeros(img.shape[:-1] + (bounds.shape[0],), dtype=img.dtype)
    for i, (x0, cnt) in enumerate(bounds):
        out[..., i] = (img[..., x0:x0 + cnt] * torch.from_numpy(coef[i, :cnt]).to(img.dtype)).sum(-1)
    return out


def resize(x, r, antialias=True, work=torch.float64):
    """[..., S, S] -> [..., r, r] in `work` (float64): the horizontal pass, then the vertical one"""
    s = x.shape[-1]
    assert x.shape[-2] == s
    b, c = resize_tables(s, r, antialias)
    h = _pass(x.to(work), b, c)
    return _pass(h.transpose(-1, -2), b, c).transpose(-1, -2)


def preprocess(x, lo, hi, r, antialias=True, work=torch.float64):
    """[B][3][S][S] in (lo, hi) -> the normalised resized images [B][3][r][r] in `work` (float64)"""
    v = resize((x.to(work) - lo) / (hi - lo), r, antialias, work)
    return (v - torch.tensor(MEAN, dtype=work).view(1, 3, 1, 1)) / torch.tensor(STD, dtype=work).view(1, 3, 1, 1)


def patch_rows(img, p):
    """normalised images [B][3][R][R] -> the ViT's patch rows [B g g][3 p^2], k = c p^2 + py p + px"""
    b, _, r, _ = img.shape
    g = r // p
    return img.reshape(b, 3, g, p, g, p).permute(0, 2, 4, 1, 3, 5).reshape(b * g * g, 3 * p * p)


# ---------------------------------------------------------------------------------------------------------------- the tower
class Prec:
    """An execution in `dtype`: every operand and result (the POINTS) is rounded to `dtype`, and the arithmetic between two points -- the sums
    inside a matrix product, a LayerNorm, a softmax, the resize -- runs in float32 (`work`), the accumulator type of every such execution, torch's
    own on the CPU included.  Rounding only whole results of float64 arithmetic would leave out what K fp32 additions inside a dot product
    cost, which for dtype float32 is most of the error.  `dtype` None: float64 throughout, nothing rounded."""
    POINTS = ("weight", "gemm_out", "norm_out", "act_out", "p", "attn_out", "embed")

    def __init__(self, dtype=None, skip=()):
        assert all(s in self.POINTS for s in skip)
        self.dtype, self.skip = dtype, set(skip)
        self.work = torch.float64 if dtype is None else torch.float32

    def r(self, x, point):
        if self.dtype is None or point in self.skip:
            return x
        return x.to(self.dtype).to(self.work)


def _ln(x, w, b):
    mu = x.mean(-1, keepdim=True)
    var = (x - mu).square().mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + LN_EPS) * w.to(x.dtype) + b.to(x.dtype)


def _lin(pr, x, w, b, res=None):
    y = x @ pr.r(w.to(pr.work), "weight").T + b.to(pr.work)
    if res is not None:
        y = y + res
    return pr.r(y, "gemm_out")


def _attention(pr, qkv, heads):
    b, n, c3 = qkv.shape
    c = c3 // 3
    q, k, v = (t.reshape(b, n, heads, c // heads).permute(0, 2, 1, 3) for t in qkv.split(c, -1))
    s = q @ k.transpose(-1, -2) * (c // heads) ** -0.5
    p = pr.r((s - s.amax(-1, keepdim=True)).exp(), "p")
    o = (p @ v) / p.sum(-1, keepdim=True)
    return pr.r(o.permute(0, 2, 1, 3).reshape(b, n, c), "attn_out")


def depth(sd):
    return len({k.split(".")[1] for k in sd if k.startswith("blocks.")})


def geometry(sd):
    w = sd["patch_embed.proj.weight"]
    g2 = sd["pos_embed"].shape[1] - 1
    return {"width": w.shape[0], "patch": w.shape[-1], "image": math.isqrt(g2) * w.shape[-1], "layers": depth(sd)}


def keys(sd, rows, b, pr=Prec()):
    """patch rows [b g g][3 p^2] -> the keys of the last block [b][1 + g^2][d]: columns d .. 2d-1 of blocks[L-1].attn.qkv's output"""
    w = sd["patch_embed.proj.weight"]
    d = w.shape[0]
    heads, layers = d // 64, depth(sd)
    pe = _lin(pr, pr.r(rows.to(pr.work), "embed"), w.reshape(d, -1), sd["patch_embed.proj.bias"]).reshape(b, -1, d)
    cls = pr.r(sd["cls_token"].to(pr.work).reshape(1, 1, d), "weight").expand(b, 1, d)
    x = pr.r(torch.cat([cls, pe], 1) + pr.r(sd["pos_embed"].to(pr.work).reshape(1, -1, d), "weight"), "embed")
    for i in range(layers):
        p = f"blocks.{i}."
        h = pr.r(_ln(x, sd[p + "norm1.weight"], sd[p + "norm1.bias"]), "norm_out")
        if i == layers - 1:
            return _lin(pr, h, sd[p + "attn.qkv.weight"][d:2 * d], sd[p + "attn.qkv.bias"][d:2 * d])
        qkv = _lin(pr, h, sd[p + "attn.qkv.weight"], sd[p + "attn.qkv.bias"])
        x = _lin(pr, _attention(pr, qkv, heads), sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"], res=x)
        h = pr.r(_ln(x, sd[p + "norm2.weight"], sd[p + "norm2.bias"]), "norm_out")
        f = _lin(pr, h, sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"])
        f = pr.r(0.5 * f * (1.0 + torch.erf(f / math.sqrt(2.0))), "act_out")
        x = _lin(pr, f, sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"], res=x)
    raise AssertionError("a tower needs at least one block")


def image_keys(sd, x, lo, hi, pr=Prec(), antialias=True):
    """[B][3][S][S] in (lo, hi) -> keys [B][n][d], float64 (an execution in pr.dtype: its values, as float64)"""
    gm = geometry(sd)
    return keys(sd, patch_rows(preprocess(x, lo, hi, gm["image"], antialias, pr.work), gm["patch"]), x.shape[0], pr).double()


# ---------------------------------------------------------------------------------------------------------------- the metric
def self_sim(k, eps=EPS):
    """keys [..., n, d] -> [..., n, n]: <k_i, k_j> / max(|k_i| |k_j|, eps); the clamp is on the product of the norms"""
    k = k.double()
    norm = k.norm(dim=-1, keepdim=True)
    return (k @ k.transpose(-1, -2)) / (norm @ norm.transpose(-1, -2)).clamp(min=eps)


def score(k_src, k_edit, eps=EPS):
    """keys [B][n][d] of the sources and of the edits -> float64 [B]: the mean over all n^2 entries of the squared difference"""
    return (self_sim(k_edit, eps) - self_sim(k_src, eps)).square().mean((-1, -2))


# ---------------------------------------------------------------------------------------------------------------- inputs
def random_state_dict(width=128, layers=3, patch=8, image=32, seed=0):
    """a DINO-shaped state dict drawn from the seed.  Matrices are int8 times a power of two with the spread of a trained layer (std about
    fan_in^-0.5): exact in fp16 and bf16, so every execution starts from the same weights."""
    g = torch.Generator().manual_seed(seed)

    def mat(*shape, std):
        e = int(round(math.log2(40.0 / std)))
        return torch.clamp((torch.randn(*shape, generator=g) * 40).round(), -127, 127) * 2.0 ** -e

    vec = lambda n, scale, one=0.0: one + scale * torch.randn(n, generator=g)
    d = width
    sd = {"cls_token": mat(1, 1, d, std=0.5), "pos_embed": mat(1, (image // patch) ** 2 + 1, d, std=0.5),
          "patch_embed.proj.weight": mat(d, 3, patch, patch, std=(3 * patch * patch) ** -0.5), "patch_embed.proj.bias": vec(d, 0.05)}
    for i in range(layers):
        p = f"blocks.{i}."
        for nm in ("norm1", "norm2"):
            sd[p + nm + ".weight"], sd[p + nm + ".bias"] = vec(d, 0.1, 1.0), vec(d, 0.05)
        sd[p + "attn.qkv.weight"], sd[p + "attn.qkv.bias"] = mat(3 * d, d, std=d ** -0.5), vec(3 * d, 0.05)
        sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"] = mat(d, d, std=d ** -0.5), vec(d, 0.05)
        sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"] = mat(4 * d, d, std=d ** -0.5), vec(4 * d, 0.05)
        sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"] = mat(d, 4 * d, std=0.5 * (4 * d) ** -0.5), vec(d, 0.05)
    sd["norm.weight"], sd["norm.bias"] = vec(d, 0.1, 1.0), vec(d, 0.05)
    return sd


def make_images(b, s, lo, hi, seed):
    """(source, edit), each (b, 3, s, s) float32 inside [lo, hi]: smooth structure plus noise; the edit moves the structure's phase and
    redraws part of the noise, so the pair is related but not equal"""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, s), torch.linspace(0, 1, s), indexing="ij")
    phase = torch.rand(b, 3, 1, 1, generator=g) * 6.28
    noise = torch.randn(b, 3, s, s, generator=g)
    src = 0.5 + 0.3 * torch.sin(7 * xx + phase) * torch.cos(5 * yy - phase) + 0.06 * noise
    shift = 0.4 + 0.8 * torch.rand(b, 1, 1, 1, generator=g)
    edit = 0.5 + 0.3 * torch.sin(7 * xx + phase + shift) * torch.cos(5 * yy - phase) + 0.06 * (0.8 * noise + 0.6 * torch.randn(b, 3, s, s, generator=g))
    f = lambda v: (lo + (hi - lo) * v.clamp(0, 1)).float().clamp(lo, hi)
    return f(src), f(edit)


def random_keys(b, n, d, dtype, seed):
    """keys [2 b][n][d] in `dtype`: rows b .. 2b-1 (edit) = rows 0 .. b-1 (source) + 0.3 noise"""
    g = torch.Generator().manual_seed(seed)
    src = torch.randn(b, n, d, generator=g)
    return torch.cat([src, src + 0.3 * torch.randn(b, n, d, generator=g)]).to(dtype)


# ---------------------------------------------------------------------------------------------------------------- the fixture's cases
# (tests/golden/make_dino_golden.py records their float64 keys, scores and yardsticks in tests/golden/dino_ref.npz; models and images are
# drawn from these seeds, not stored)
MODELS = {"a": dict(width=128, layers=3, patch=8, image=32, seed=11), "b": dict(width=128, layers=2, patch=8, image=224, seed=12)}
CASES = {"a20": dict(model="a", pairs=8, s=20, seed=201, stride=2), "a64": dict(model="a", pairs=8, s=64, seed=202, stride=4),
         "b": dict(model="b", pairs=2, s=256, seed=203, stride=16), "syn": dict(model="syn", pairs=8, s=20, seed=201, stride=4)}
E2E = dict(width=384, layers=12, patch=8, image=224, seed=13, s=240, image_seed=204)


def case_state_dict(model):
    """"a" / "b": drawn from the seed; "syn": the library's synthetic weights at its "tiny/8" geometry (the one import of the library here)"""
    if model == "syn":
        from etainv.weights import synthetic_dino_state_dict
        from metrics.dino_vit_structure import GEOMETRY
        return synthetic_dino_state_dict(**GEOMETRY["tiny/8"])
    return random_state_dict(**MODELS[model])


def case_inputs(case):
    """(state dict, images [2 pairs][3][s][s] = sources then edits in (-1, 1), pairs)"""
    c = CASES[case]
    src, edit = make_images(c["pairs"], c["s"], -1, 1, c["seed"])
    return case_state_dict(c["model"]), torch.cat([src, edit]), c["pairs"]
