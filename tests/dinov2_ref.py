"""References for the dinovitstruct_v2 metric (torch and numpy only; no import of the library but for the "syn" case's weights, none of
transformers): what DINOv2 adds over the DINO tower of tests/dino_ref.py, restated from the published `vision_transformer.py` of
facebookresearch/dinov2 (`DinoVisionTransformer.interpolate_pos_encoding`, `Block`, `LayerScale`; the hub is not reachable from a test, so
nothing is imported from it):

  patch 14       `PatchEmbed`: Conv2d(3, d, 14, 14) with bias; the preprocessing is the reference metric's own (Resize(224), ImageNet normalisation),
                 so a square image gives 16 x 16 patches and n = 257 tokens
  position table `pos_embed` is [1][1 + M M][d] (M = 37: trained at 518).  For a g x g grid, g != M, the model takes the M x M patch part in
                 float32 through F.interpolate(mode="bicubic", antialias=False, scale_factor=((g + o) / M, (g + o) / M)) with
                 o = interpolate_offset = 0.1 (the default of the hub's non-register models), and prepends the class row unchanged.  With
                 scale_factor given torch maps output to input coordinates with 1 / scale_factor, not with M / g.  o = 0: size=(g, g), the form
                 of transformers' Dinov2Model.  `bicubic_weights` restates torch's bicubic kernel: A = -0.75, taps floor(s) - 1 .. floor(s) + 2
                 with indices clamped to [0, M - 1], s = (i + 0.5) scale - 0.5 (not clamped at 0).
  LayerScale     x = x + ls1.gamma * attn(norm1(x)); x = x + ls2.gamma * mlp(norm2(x)); gamma [d] per block and branch.
                 LayerNorm eps 1e-6, erf GELU, heads = d / 64 (vits14 384, vitb14 768, vitl14 1024).
The 0.1 offset is taken from that published code and cannot be checked against it where the tests run; tests/test_dinov2_ref.py pins the
restatement against F.interpolate in both forms and the o = 0 tower against transformers' Dinov2Model.

The tower runs on dino_ref's `Prec`: the rounding points of a 16-bit execution.  The fused residual step rounds x + gamma * y once (the stored
residual stream) and the LayerNorm of that stored value once; gamma stays float32 / float64 and is never folded into rounded weights."""
import math

import torch

from tests import dino_ref as dr
from tests.dino_ref import Prec, make_images, patch_rows, preprocess, score, self_sim  # noqa: F401  (re-exported for the tests)

PATCH = 14
A = -0.75


# ---------------------------------------------------------------------------------------------------------------- the position table
def bicubic_weights(m, g, scale, work=torch.float64):
    """[g][m] in `work`: row i holds the four cubic-convolution weights of output i at the (clamped, hence possibly coinciding) input indices;
    `scale` maps output to input coordinates (1 / scale_factor, or m / g for size=)"""
    w = torch.zeros(g, m, dtype=work)
    c1 = lambda t: ((A + 2) * t - (A + 3)) * t * t + 1            # |t| <= 1
    c2 = lambda t: ((A * t - 5 * A) * t + 8 * A) * t - 4 * A      # 1 < |t| < 2
    for i in range(g):
        s = torch.tensor((i + 0.5) * scale - 0.5, dtype=work)
        f = torch.floor(s)
        t = s - f
        for k, c in zip(range(-1, 3), (c2(t + 1), c1(t), c1(1 - t), c2(2 - t))):
            w[i, min(max(int(f) + k, 0), m - 1)] += c
    return w


def position_table(pos_embed, g, offset=0.1, work=torch.float64):
    """pos_embed [1][1 + M M][d] -> [1 + g g][d] in `work`: the class row, then the interpolated grid, row-major"""
    pos = pos_embed.to(work).reshape(-1, pos_embed.shape[-1])
    m = math.isqrt(pos.shape[0] - 1)
    if g == m:
        return pos
    scale = 1.0 / (float(g + offset) / m) if offset else m / g
    w = bicubic_weights(m, g, scale, work)
    grid = pos[1:].reshape(m, m, -1)
    out = torch.einsum("ia,jb,abd->ijd", w, w, grid)
    return torch.cat([pos[:1], out.reshape(g * g, -1)])


# ---------------------------------------------------------------------------------------------------------------- the tower
def geometry(sd, image=None):
    w = sd["patch_embed.proj.weight"]
    m = math.isqrt(sd["pos_embed"].shape[1] - 1)
    image = image if image is not None else (224 if m >= 16 else m * PATCH)
    return {"width": w.shape[0], "patch": PATCH, "image": image, "table": m, "layers": dr.depth(sd)}


def keys(sd, rows, b, pr=Prec(), offset=0.1, table=None):
    """patch rows [b g g][588] -> the keys of the last block [b][1 + g g][d]; `table`: a position table [1 + g g][d] to use instead of
    position_table's"""
    w = sd["patch_embed.proj.weight"]
    d = w.shape[0]
    heads, layers, g = d // 64, dr.depth(sd), math.isqrt(rows.shape[0] // b)
    lin, ln = dr._lin, dr._ln
    pe = lin(pr, pr.r(rows.to(pr.work), "embed"), w.reshape(d, -1), sd["patch_embed.proj.bias"]).reshape(b, -1, d)
    cls = pr.r(sd["cls_token"].to(pr.work).reshape(1, 1, d), "weight").expand(b, 1, d)
    table = position_table(sd["pos_embed"], g, offset, pr.work) if table is None else table.to(pr.work)
    x = pr.r(torch.cat([cls, pe], 1) + pr.r(table[None], "weight"), "embed")
    h = pr.r(ln(x, sd["blocks.0.norm1.weight"], sd["blocks.0.norm1.bias"]), "norm_out")
    for i in range(layers):
        p = f"blocks.{i}."
        if i == layers - 1:
            return lin(pr, h, sd[p + "attn.qkv.weight"][d:2 * d], sd[p + "attn.qkv.bias"][d:2 * d])
        qkv = lin(pr, h, sd[p + "attn.qkv.weight"], sd[p + "attn.qkv.bias"])
        y = lin(pr, dr._attention(pr, qkv, heads), sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"])
        x = pr.r(x + sd[p + "ls1.gamma"].to(pr.work) * y, "gemm_out")                                # the fused step: x_out once ...
        h = pr.r(ln(x, sd[p + "norm2.weight"], sd[p + "norm2.bias"]), "norm_out")                    # ... h_out once
        f = lin(pr, h, sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"])
        f = pr.r(0.5 * f * (1.0 + torch.erf(f / math.sqrt(2.0))), "act_out")
        y = lin(pr, f, sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"])
        x = pr.r(x + sd[p + "ls2.gamma"].to(pr.work) * y, "gemm_out")
        q = f"blocks.{i + 1}."
        h = pr.r(ln(x, sd[q + "norm1.weight"], sd[q + "norm1.bias"]), "norm_out")
    raise AssertionError("a tower needs at least one block")


def image_keys(sd, x, lo, hi, pr=Prec(), antialias=True, offset=0.1, image=None):
    """[B][3][S][S] in (lo, hi) -> keys [B][n][d], float64 (an execution in pr.dtype: its values, as float64)"""
    gm = geometry(sd, image)
    return keys(sd, patch_rows(preprocess(x, lo, hi, gm["image"], antialias, pr.work), PATCH), x.shape[0], pr, offset).double()


# ---------------------------------------------------------------------------------------------------------------- inputs
def random_state_dict(width=128, layers=3, table=5, seed=0):
    """a DINOv2-shaped state dict drawn from the seed: dino_ref's recipe (matrices int8 times a power of two, exact in fp16 and bf16) over an
    M x M position table, plus LayerScale gammas that are powers of two from 2^-17 to 1 with random sign (exact in every type, spanning the
    range trained gammas do)"""
    sd = dr.random_state_dict(width=width, layers=layers, patch=PATCH, image=table * PATCH, seed=seed)
    g = torch.Generator().manual_seed(seed + 7919)
    for i in range(layers):
        for nm in ("ls1", "ls2"):
            e = torch.randint(-17, 1, (width,), generator=g).double()
            sign = torch.randint(0, 2, (width,), generator=g).double() * 2 - 1
            sd[f"blocks.{i}.{nm}.gamma"] = (sign * torch.pow(2.0, e)).float()
    sd["mask_token"] = torch.zeros(1, width)
    return sd


# ---------------------------------------------------------------------------------------------------------------- the fixture's cases
# (tests/golden/make_dinov2_golden.py records their float64 keys, scores and yardsticks in tests/golden/dinov2_ref.npz)
MODELS = {"a": dict(width=128, layers=3, table=5, seed=21, image=42), "b": dict(width=128, layers=2, table=37, seed=22, image=224)}
CASES = {"a20": dict(model="a", pairs=8, s=20, seed=301, stride=1), "a64": dict(model="a", pairs=8, s=64, seed=302, stride=1),
         "b": dict(model="b", pairs=2, s=256, seed=303, stride=16), "syn": dict(model="syn", pairs=8, s=20, seed=301, stride=1)}
E2E = dict(width=384, layers=12, table=37, seed=23, s=240, image_seed=304)


def case_model(model):
    """(state dict, image side): "a" / "b" drawn from the seed; "syn": the library's synthetic weights at "tinyv2/14" (the one import of the library)"""
    if model == "syn":
        from etainv.weights import synthetic_dinov2_state_dict
        from metrics.dino_vit_structure import GEOMETRY_V2
        return synthetic_dinov2_state_dict(**GEOMETRY_V2["tinyv2/14"]), GEOMETRY_V2["tinyv2/14"]["image"]
    m = MODELS[model]
    return random_state_dict(m["width"], m["layers"], m["table"], m["seed"]), m["image"]


def case_inputs(case):
    """(state dict, image side, images [2 pairs][3][s][s] = sources then edits in (-1, 1), pairs)"""
    c = CASES[case]
    src, edit = make_images(c["pairs"], c["s"], -1, 1, c["seed"])
    sd, image = case_model(c["model"])
    return sd, image, torch.cat([src, edit]), c["pairs"]
