"""References for the CLIP metrics (torch and numpy only; no import of the library, none of transformers): Pillow's bicubic resize restated in
integer arithmetic, CLIP's image preprocessing, float64 vision and text towers over transformers' `CLIPModel` state-dict names, the embedding
head, the four scores, an emulation of what a 16-bit execution must round, and input builders.
tests/test_clip_ref.py pins these helpers on the CPU (against Pillow and transformers themselves); the GPU tests use them."""
import math

import numpy as np
import torch

MEAN = (0.48145466, 0.4578275, 0.40821073)      # the published normalisation constants of CLIP
STD = (0.26862954, 0.26130258, 0.27577711)
PRECISION_BITS = 22
MODES = ("text_img", "img_img", "textdir_imgdir", "text_img_acc")


# ---------------------------------------------------------------------------------------------------------------- Pillow's resize
def bicubic(x, a=-0.5):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def resize_tables(n_in, n_out):
    """(bounds [n_out][2] = (first tap, taps), coef [n_out][ksize] int32): Pillow's precompute_coeffs + normalize_coeffs_8bpc for the bicubic
    filter.  n_in == n_out: one tap of weight 2^22 (Pillow returns the image unresampled)."""
    if n_in == n_out:
        bounds = np.stack([np.arange(n_out), np.ones(n_out, dtype=np.int64)], 1).astype(np.int32)
        return bounds, np.full((n_out, 1), 1 << PRECISION_BITS, dtype=np.int32)
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((n_out, 2), dtype=np.int32)
    coef = np.zeros((n_out, ksize), dtype=np.int32)
    for i in range(n_out):
        center = (i + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in)
        w = [bicubic((j + xmin - center + 0.5) / fs) for j in range(xmax - xmin)]
        total = 0.0
        for v in w:
            total += v
        bounds[i] = (xmin, xmax - xmin)
        for j, v in enumerate(w):
            v = v / total
            coef[i, j] = int(v * (1 << PRECISION_BITS) + (0.5 if v >= 0 else -0.5))
    return bounds, coef


def _pass(img, bounds, coef):
    """one resampling pass along the last axis of a uint8 array"""
    out = np.empty(img.shape[:-1] + (bounds.shape[0],), dtype=np.uint8)
    src = img.astype(np.int64)
    for i, (x0, cnt) in enumerate(bounds):
        acc = (1 << (PRECISION_BITS - 1)) + (src[..., x0:x0 + cnt] * coef[i, :cnt].astype(np.int64)).sum(-1)
        out[..., i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def pillow_resize_u8(img, r):
    """uint8 [..., S, S] -> uint8 [..., r, r]: the horizontal pass into uint8, then the vertical pass"""
    s = img.shape[-1]
    assert img.dtype == np.uint8 and img.shape[-2] == s
    if s == r:
        return img.copy()
    b, c = resize_tables(s, r)
    h = _pass(img, b, c)
    return np.swapaxes(_pass(np.swapaxes(h, -1, -2), b, c), -1, -2)


def to_u8(x, lo, hi):
    """torch_to_pil: float32 arithmetic, clamp, truncation"""
    v = (x.float() - lo) / (hi - lo)
    return np.clip(v.numpy() * 255, 0, 255).astype(np.uint8)


def k_padded(p):
    return (3 * p * p + 63) // 64 * 64


def preprocess_u8(x, lo, hi, r):
    return pillow_resize_u8(to_u8(x, lo, hi), r)


def patch_rows(u8, p, dtype=torch.float64):
    """resized bytes [B][3][R][R] -> the ViT's patch rows [B g g][Kp] (k = c p^2 + py p + px, zero padding), normalised in float64"""
    b, _, r, _ = u8.shape
    g = r // p
    v = torch.from_numpy(u8.astype(np.float64)) / 255.0
    v = (v - torch.tensor(MEAN, dtype=torch.float64).view(1, 3, 1, 1)) / torch.tensor(STD, dtype=torch.float64).view(1, 3, 1, 1)
    rows = v.reshape(b, 3, g, p, g, p).permute(0, 2, 4, 1, 3, 5).reshape(b * g * g, 3 * p * p)
    out = torch.zeros(b * g * g, k_padded(p), dtype=torch.float64)
    out[:, :3 * p * p] = rows
    return out.to(dtype)


# ---------------------------------------------------------------------------------------------------------------- towers
class Prec:
    """Where a 16-bit execution rounds: `dtype` None = float64 throughout.  `skip`: names of rounding points left out (a deliberately broken
    emulation: tests/test_clip_ref.py)."""
    POINTS = ("weight", "gemm_out", "norm_out", "act_out", "p", "attn_out", "embed")

    def __init__(self, dtype=None, skip=()):
        assert all(s in self.POINTS for s in skip)
        self.dtype, self.skip = dtype, set(skip)

    def r(self, x, point):
        if self.dtype is None or point in self.skip:
            return x
        return x.to(self.dtype).double()


def _ln(x, w, b, eps=1e-5):
    mu = x.mean(-1, keepdim=True)
    var = (x - mu).square().mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w.double() + b.double()


def _lin(pr, x, w, b=None, res=None):
    y = x @ pr.r(w.double(), "weight").T                   # (x is some rounding point's output already)
    if b is not None:
        y = y + b.double()
    if res is not None:
        y = y + res
    return pr.r(y, "gemm_out")


def _attention(pr, q, k, v, heads, causal):
    b, n, c = q.shape
    d = c // heads
    sp = lambda t: t.reshape(b, n, heads, d).permute(0, 2, 1, 3)
    s = sp(q) @ sp(k).transpose(-1, -2) * d ** -0.5
    if causal:
        s = s + torch.full((n, n), float("-inf"), dtype=torch.float64).triu(1)
    p = pr.r((s - s.amax(-1, keepdim=True)).exp(), "p")
    o = (p @ sp(v)) / p.sum(-1, keepdim=True)
    return pr.r(o.permute(0, 2, 1, 3).reshape(b, n, c), "attn_out")


def _encoder(pr, sd, pre, x, heads, causal):
    i = 0
    while f"{pre}encoder.layers.{i}.layer_norm1.weight" in sd:
        p = f"{pre}encoder.layers.{i}."
        h = pr.r(_ln(x, sd[p + "layer_norm1.weight"], sd[p + "layer_norm1.bias"]), "norm_out")
        q, k, v = (_lin(pr, h, sd[p + f"self_attn.{n}.weight"], sd[p + f"self_attn.{n}.bias"]) for n in ("q_proj", "k_proj", "v_proj"))
        x = _lin(pr, _attention(pr, q, k, v, heads, causal), sd[p + "self_attn.out_proj.weight"], sd[p + "self_attn.out_proj.bias"], res=x)
        h = pr.r(_ln(x, sd[p + "layer_norm2.weight"], sd[p + "layer_norm2.bias"]), "norm_out")
        f = _lin(pr, h, sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"])
        f = pr.r(f * torch.sigmoid(1.702 * f), "act_out")
        x = _lin(pr, f, sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"], res=x)
        i += 1
    return x


def geometry(sd):
    w = sd["vision_model.embeddings.patch_embedding.weight"]
    d, p = w.shape[0], w.shape[-1]
    g2 = sd["vision_model.embeddings.position_embedding.weight"].shape[0] - 1
    return {"width": d, "patch": p, "image": int(round(math.sqrt(g2))) * p, "proj": sd["visual_projection.weight"].shape[0],
            "text_width": sd["text_model.embeddings.token_embedding.weight"].shape[1]}


def head(x_row, ln, proj, normalize=True):
    """pooled row(s) [B][d] -> optional LayerNorm (weight, bias) -> projection [P][d] -> unit vectors (normalize=False: as projected), float64"""
    x = x_row.double()
    if ln is not None:
        x = _ln(x, ln[0], ln[1])
    e = x @ proj.double().T
    return e / e.norm(dim=-1, keepdim=True) if normalize else e


def vision_hidden(sd, rows, b, pr=Prec()):
    """patch rows [b g g][Kp] -> the encoder's output [b][1 + g^2][d] (before post_layernorm)"""
    pre = "vision_model."
    w = sd[pre + "embeddings.patch_embedding.weight"]
    d = w.shape[0]
    w2 = torch.zeros(d, rows.shape[1], dtype=torch.float64)
    w2[:, :w[0].numel()] = w.reshape(d, -1).double()
    pe = _lin(pr, pr.r(rows.double(), "embed"), w2).reshape(b, -1, d)
    cls = pr.r(sd[pre + "embeddings.class_embedding"].double(), "weight").expand(b, 1, d)
    x = torch.cat([cls, pe], 1) + pr.r(sd[pre + "embeddings.position_embedding.weight"].double(), "weight")
    x = pr.r(x, "embed")
    x = pr.r(_ln(x, sd[pre + "pre_layrnorm.weight"], sd[pre + "pre_layrnorm.bias"]), "norm_out")
    return _encoder(pr, sd, pre, x, d // 64, False)


def image_features(sd, rows, b, pr=Prec(), normalize=True):
    x = vision_hidden(sd, rows, b, pr)
    return head(x[:, 0], (sd["vision_model.post_layernorm.weight"], sd["vision_model.post_layernorm.bias"]), sd["visual_projection.weight"], normalize)


def text_features(sd, ids, pr=Prec(), normalize=True):
    """ids [B][n] int64 -> unit embeddings [B][P]; pooled at argmax(ids) (OpenAI's rule)"""
    pre = "text_model."
    tok = pr.r(sd[pre + "embeddings.token_embedding.weight"].double(), "weight")
    pos = pr.r(sd[pre + "embeddings.position_embedding.weight"].double(), "weight")
    x = pr.r(tok[ids] + pos[: ids.shape[1]], "embed")
    x = _encoder(pr, sd, pre, x, tok.shape[1] // 64, True)
    x = pr.r(_ln(x, sd[pre + "final_layer_norm.weight"], sd[pre + "final_layer_norm.bias"]), "norm_out")
    return head(x[torch.arange(ids.shape[0]), ids.argmax(-1)], None, sd["text_projection.weight"], normalize)


# ---------------------------------------------------------------------------------------------------------------- scores
def prompt_embedding(e):
    """[B][T][P] unit embeddings of a prompt's T captions -> [B][P]: their mean, renormalised"""
    m = e.double().mean(1)
    return m / m.norm(dim=-1, keepdim=True)


def scores(mode, img_src=None, img_tgt=None, txt_src=None, txt_tgt=None):
    """float64 [B]; img_* [B][P], txt_* [B][T][P]"""
    d = lambda t: t.double()
    if mode == "text_img":
        return (d(img_tgt) * prompt_embedding(txt_tgt)).sum(-1)
    if mode == "img_img":
        return (d(img_src) * d(img_tgt)).sum(-1)
    if mode == "textdir_imgdir":
        return ((d(img_tgt) - d(img_src)) * (prompt_embedding(txt_tgt) - prompt_embedding(txt_src))).sum(-1)
    assert mode == "text_img_acc"
    return ((d(img_tgt) * prompt_embedding(txt_tgt)).sum(-1) > (d(img_tgt) * prompt_embedding(txt_src)).sum(-1)).double()


# ---------------------------------------------------------------------------------------------------------------- inputs
def make_images(b, s, lo, hi, seed):
    """(b, 3, s, s) float32: smooth structure plus noise, reaching below lo and above hi"""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, s), torch.linspace(0, 1, s), indexing="ij")
    phase = torch.rand(b, 3, 1, 1, generator=g) * 6.28
    base = 0.5 + 0.45 * torch.sin(7 * xx + phase) * torch.cos(5 * yy - phase) + 0.25 * torch.randn(b, 3, s, s, generator=g)
    return (lo + (hi - lo) * base).float()


def truncation_images(s, lo, hi):
    """(1, 3, s, s): values that map to k + 0.999 for k cycling through 0 .. 254: truncation gives k, rounding k + 1"""
    k = (torch.arange(3 * s * s) % 255).double()
    return (lo + (hi - lo) * (k + 0.999) / 255.0).float().reshape(1, 3, s, s)


def unit_rows(shape, seed):
    g = torch.Generator().manual_seed(seed)
    e = torch.randn(shape, generator=g, dtype=torch.float64)
    return (e / e.norm(dim=-1, keepdim=True)).float()


def random_state_dict(width=128, layers=2, patch=16, image=32, proj=64, text_width=128, text_layers=2, vocab=64, seed=0):
    """a CLIPModel-shaped state dict of small random tensors (transformers' names)"""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s, scale=1.0: torch.randn(*s, generator=g) * scale
    sd = {}

    def enc(pre, d, n):
        for i in range(n):
            p = f"{pre}encoder.layers.{i}."
            for nm in ("q_proj", "k_proj", "v_proj", "out_proj"):
                sd[p + f"self_attn.{nm}.weight"], sd[p + f"self_attn.{nm}.bias"] = rn(d, d, scale=d ** -0.5), rn(d, scale=0.05)
            for nm in ("layer_norm1", "layer_norm2"):
                sd[p + nm + ".weight"], sd[p + nm + ".bias"] = 1 + rn(d, scale=0.1), rn(d, scale=0.05)
            sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"] = rn(4 * d, d, scale=d ** -0.5), rn(4 * d, scale=0.05)
            sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"] = rn(d, 4 * d, scale=0.5 * (4 * d) ** -0.5), rn(d, scale=0.05)

    v = "vision_model."
    sd[v + "embeddings.class_embedding"] = rn(width, scale=0.5)
    sd[v + "embeddings.patch_embedding.weight"] = rn(width, 3, patch, patch, scale=(3 * patch * patch) ** -0.5)
    sd[v + "embeddings.position_embedding.weight"] = rn((image // patch) ** 2 + 1, width, scale=0.5)
    for nm in ("pre_layrnorm", "post_layernorm"):
        sd[v + nm + ".weight"], sd[v + nm + ".bias"] = 1 + rn(width, scale=0.1), rn(width, scale=0.05)
    enc(v, width, layers)
    t = "text_model."
    sd[t + "embeddings.token_embedding.weight"] = rn(vocab, text_width, scale=0.5)
    sd[t + "embeddings.position_embedding.weight"] = rn(77, text_width, scale=0.5)
    sd[t + "final_layer_norm.weight"], sd[t + "final_layer_norm.bias"] = 1 + rn(text_width, scale=0.1), rn(text_width, scale=0.05)
    enc(t, text_width, text_layers)
    sd["visual_projection.weight"] = rn(proj, width, scale=width ** -0.5)
    sd["text_projection.weight"] = rn(proj, text_width, scale=text_width ** -0.5)
    sd["logit_scale"] = torch.tensor(2.6592)
    return sd
