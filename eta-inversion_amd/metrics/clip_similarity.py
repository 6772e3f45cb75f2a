"""The CLIP metrics (reference metrics/clip_similarity.py:160-324): `CLIPSimilarity`, `CLIPAccuracy` and `clip_scores`, the batched call they sit on.

Device tensors go to the HIP kernels (csrc/clip.hip and the towers of etainv/nets.py: one preprocess launch for the 2 B images, one pass per
tower, one score launch per metric).  CPU tensors, or device="cpu", go to the plain-torch float32 path below, which keeps the package and
compute_metrics.py usable without a GPU.  Both run the same steps: torch_to_pil (:223-239: normalise, * 255, clamp, truncate to a byte), clip's
transform (:201: Pillow's bicubic resize on bytes, restated in integer arithmetic; / 255, - mean, / std), the towers, the division by the norm
(:205, :120), the template average (:118-125) and the dot products (:257-273, :317-321).

Weights are handed over explicitly (`weights=`: a path, a state dict, a loaded `ClipModel`, or "synthetic"); there is no default and no environment
variable.  The list of caption templates is the caller's (`templates=`): none is shipped.  `text_text` needs a BLIP captioner and is refused.
Images must be square: the smaller-edge resize plus centre crop of clip's transform is the identity on them."""
import functools
import math
import os
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch
import torch.nn.functional as F

from .base import SimpleMetric

MEAN = (0.48145466, 0.4578275, 0.40821073)          # the published normalisation constants of CLIP
STD = (0.26862954, 0.26130258, 0.27577711)
MODES = ("text_img", "img_img", "textdir_imgdir", "text_img_acc")
CONTEXT = 77
GEOMETRY = {
    "ViT-B/32": dict(width=768, layers=12, patch=32, image=224, proj=512, text_width=512, text_layers=12),
    "ViT-B/16": dict(width=768, layers=12, patch=16, image=224, proj=512, text_width=512, text_layers=12),
    "ViT-L/14": dict(width=1024, layers=24, patch=14, image=224, proj=768, text_width=768, text_layers=12),
    "tiny/16": dict(width=128, layers=2, patch=16, image=32, proj=64, text_width=128, text_layers=2),   # synthetic weights only: quick runs
}
_BLIP = "needs a BLIP captioner (reference metrics/clip_similarity.py:128-157), which is not built"


class PromptTooLong(RuntimeError):
    pass


# ---------------------------------------------------------------------------------------------------------------- Pillow's bicubic resize
def _bicubic(x: float) -> float:
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


@functools.lru_cache(maxsize=16)
def resize_tables(n_in: int, n_out: int) -> Tuple[np.ndarray, np.ndarray]:
    """(read-only, cached per size pair) (bounds [n_out][2] = (first tap, taps), coef [n_out][ksize]) int32: the bicubic coefficients as Pillow builds them, in float64, normalised
    to sum 1 and converted to 22-bit fixed point as int(w 2^22 +- 0.5).  n_in == n_out: one tap of weight 2^22 (Pillow does not resample)."""
    if n_in == n_out:
        return (np.stack([np.arange(n_out), np.ones(n_out, dtype=np.int64)], 1).astype(np.int32), np.full((n_out, 1), 1 << 22, dtype=np.int32))
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 2.0 * fs
    bounds = np.zeros((n_out, 2), dtype=np.int32)
    coef = np.zeros((n_out, int(math.ceil(support)) * 2 + 1), dtype=np.int32)
    for i in range(n_out):
        center = (i + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in)
        w = [_bicubic((j + xmin - center + 0.5) / fs) for j in range(xmax - xmin)]
        total = 0.0
        for v in w:
            total += v
        bounds[i] = (xmin, xmax - xmin)
        coef[i, :len(w)] = [int(v / total * 4194304.0 + (0.5 if v / total >= 0 else -0.5)) for v in w]
    bounds.setflags(write=False)
    coef.setflags(write=False)
    return bounds, coef


@functools.lru_cache(maxsize=16)
def _device_tables(n_in: int, n_out: int, p: int, device: str):
    """the tables of `resize_tables` on the device, with their tap count and the band height: built and copied once per (sizes, device)"""
    bounds, coef = resize_tables(n_in, n_out)
    return (torch.from_numpy(bounds.copy()).to(device), torch.from_numpy(coef.copy()).to(device), coef.shape[1], _band_rows(bounds, p))


def _band_rows(bounds: np.ndarray, p: int) -> int:
    """the most input rows a band of p output rows spans"""
    first, last = bounds[0::p], bounds[p - 1::p]
    return int((last[:, 0] + last[:, 1] - first[:, 0]).max())


def _k_padded(p: int) -> int:
    return (3 * p * p + 63) // 64 * 64


def _check_images(x: torch.Tensor, r: int, p: int) -> None:
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f"Input images should be (B, 3, H, W) tensors, but got {tuple(x.shape)}")
    if x.shape[2] != x.shape[3]:
        raise ValueError(f"the CLIP metrics take square images (the smaller-edge resize plus centre crop is not built), but got {tuple(x.shape[2:])}")
    if p not in (14, 16, 32) or r % p:
        raise ValueError(f"patch size {p} must be 14, 16 or 32 and divide the model's image size {r}")


def _range(input_range) -> Tuple[float, float]:
    lo, hi = (0.0, 1.0) if input_range is None else (float(input_range[0]), float(input_range[1]))
    if not hi > lo:
        raise ValueError(f"input_range must be (lo, hi) with hi > lo, got {input_range}")
    return lo, hi


def _resample_torch(img: torch.Tensor, bounds: np.ndarray, coef: np.ndarray) -> torch.Tensor:
    """one pass along the last axis: int32 [..., n_in] -> int32 [..., n_out] bytes"""
    n_in, ks = img.shape[-1], coef.shape[1]
    j = torch.arange(ks)
    b = torch.from_numpy(bounds.astype(np.int64))
    idx = (b[:, :1] + j).clamp_(max=n_in - 1)                                   # [n_out][ks]; taps beyond the count carry weight 0
    w = torch.from_numpy(coef.astype(np.int64)) * (j < b[:, 1:2])
    acc = (img.long()[..., idx] * w).sum(-1) + (1 << 21)
    return (acc >> 22).clamp_(0, 255).to(torch.int32)


def _preprocess_torch(x: torch.Tensor, lo: float, hi: float, r: int, p: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(patch rows float32 [B g g][Kp], resized bytes uint8 [B][3][r][r]).  The bytes equal the kernel's; the normalisation runs in the three
    float32 steps of ToTensor + Normalize, where the kernel normalises in float64 and rounds once: a row may differ from the device's by about
    1e-7 absolute."""
    b, s, g = x.shape[0], x.shape[-1], r // p
    bounds, coef = resize_tables(s, r)
    out = torch.empty(b, 3, r, r, dtype=torch.uint8)
    for i in range(b):
        u8 = (((x[i].float() - lo) / (hi - lo)) * 255).clamp_(0, 255).to(torch.uint8).to(torch.int32)
        h = _resample_torch(u8, bounds, coef)
        out[i] = _resample_torch(h.transpose(-1, -2), bounds, coef).transpose(-1, -2).to(torch.uint8)
    v = (out.float() / 255.0 - torch.tensor(MEAN).view(1, 3, 1, 1)) / torch.tensor(STD).view(1, 3, 1, 1)
    rows = torch.zeros(b * g * g, _k_padded(p))
    rows[:, :3 * p * p] = v.reshape(b, 3, g, p, g, p).permute(0, 2, 4, 1, 3, 5).reshape(b * g * g, 3 * p * p)
    return rows, out


def clip_preprocess(x: torch.Tensor, input_range=(-1, 1), r: int = 224, p: int = 16, dtype=torch.float16, return_u8: bool = False):
    """(B, 3, S, S) images in `input_range` -> the ViT's patch rows [B (r / p)^2][Kp] in `dtype` (element k = c p^2 + py p + px, zero beyond
    3 p^2); with return_u8 also the resized bytes (B, 3, r, r).  Device tensors: one etainv_clip_preprocess launch; CPU tensors: float32 torch."""
    _check_images(x, r, p)
    lo, hi = _range(input_range)
    if not x.is_cuda:
        rows, u8 = _preprocess_torch(x.detach(), lo, hi, r, p)
        return (rows.to(dtype), u8) if return_u8 else rows.to(dtype)
    from etainv import _capi
    lib = _capi.load()
    x = x.detach().to(torch.float32).contiguous()
    b, s, g = x.shape[0], x.shape[-1], r // p
    tb, tc, ksize, band = _device_tables(s, r, p, str(x.device))
    with torch.cuda.device(x.device):
        rows = torch.empty(b * g * g, _k_padded(p), dtype=dtype, device=x.device)
        u8 = torch.empty(b, 3, r, r, dtype=torch.uint8, device=x.device) if return_u8 else None
        _capi.check(lib.etainv_clip_preprocess(_capi.ptr(x), b, s, r, p, lo, hi, _capi.ptr(tb), _capi.ptr(tc), ksize, _capi.ptr(tb),
                                               _capi.ptr(tc), ksize, band, _capi.ptr(rows), _capi.ptr(u8),
                                               _capi.dtype_code(dtype), _capi.stream_ptr()))
    return (rows, u8) if return_u8 else rows


# ---------------------------------------------------------------------------------------------------------------- the float32 torch towers
class _TorchCLIP:
    """the towers in plain float32 torch on the CPU, over transformers' `CLIPModel` state-dict names"""

    def __init__(self, sd: dict):
        from etainv.nets import clip_geometry
        self.sd = {k: v.float() for k, v in sd.items()}
        gm = clip_geometry(sd)
        self.patch, self.image, self.proj, self.vocab = gm["patch"], gm["image"], gm["proj"], gm["vocab"]
        self.heads = {"vision_model.": gm["width"] // 64, "text_model.": gm["text_width"] // 64}
        self.layers = {"vision_model.": gm["layers"], "text_model.": gm["text_layers"]}

    def _encoder(self, pre: str, x: torch.Tensor, causal: bool) -> torch.Tensor:
        sd, heads = self.sd, self.heads[pre]
        b, n, c = x.shape
        mask = torch.full((n, n), float("-inf")).triu(1) if causal else None
        sp = lambda t: t.reshape(b, n, heads, c // heads).transpose(1, 2)
        lin = lambda t, name: F.linear(t, sd[name + ".weight"], sd[name + ".bias"])
        for i in range(self.layers[pre]):
            p = f"{pre}encoder.layers.{i}."
            h = F.layer_norm(x, (c,), sd[p + "layer_norm1.weight"], sd[p + "layer_norm1.bias"])
            q, k, v = (sp(lin(h, p + "self_attn." + nm)) for nm in ("q_proj", "k_proj", "v_proj"))
            s = q @ k.transpose(-1, -2) * (c // heads) ** -0.5
            a = (s if mask is None else s + mask).softmax(-1) @ v
            x = x + lin(a.transpose(1, 2).reshape(b, n, c), p + "self_attn.out_proj")
            f = lin(F.layer_norm(x, (c,), sd[p + "layer_norm2.weight"], sd[p + "layer_norm2.bias"]), p + "mlp.fc1")
            x = x + lin(f * torch.sigmoid(1.702 * f), p + "mlp.fc2")
        return x

    def image_features(self, rows: torch.Tensor, b: int) -> torch.Tensor:
        sd, pre = self.sd, "vision_model."
        w = sd[pre + "embeddings.patch_embedding.weight"]
        d, k = w.shape[0], w[0].numel()
        pe = (rows.float()[:, :k] @ w.reshape(d, k).T).reshape(b, -1, d)
        x = torch.cat([sd[pre + "embeddings.class_embedding"].expand(b, 1, d), pe], 1) + sd[pre + "embeddings.position_embedding.weight"]
        x = F.layer_norm(x, (d,), sd[pre + "pre_layrnorm.weight"], sd[pre + "pre_layrnorm.bias"])
        x = self._encoder(pre, x, False)[:, 0]
        e = F.layer_norm(x, (d,), sd[pre + "post_layernorm.weight"], sd[pre + "post_layernorm.bias"]) @ sd["visual_projection.weight"].T
        return e / e.norm(dim=-1, keepdim=True)

    def text_features(self, ids: torch.Tensor) -> torch.Tensor:
        sd, pre = self.sd, "text_model."
        ids = ids.cpu()
        if int(ids.max()) >= self.vocab or int(ids.min()) < 0:
            raise ValueError(f"token id outside the vocabulary of {self.vocab} entries")
        x = sd[pre + "embeddings.token_embedding.weight"][ids] + sd[pre + "embeddings.position_embedding.weight"][: ids.shape[1]]
        x = self._encoder(pre, x, True)
        x = F.layer_norm(x, x.shape[-1:], sd[pre + "final_layer_norm.weight"], sd[pre + "final_layer_norm.bias"])
        e = x[torch.arange(ids.shape[0]), ids.argmax(-1)] @ sd["text_projection.weight"].T
        return e / e.norm(dim=-1, keepdim=True)


# ---------------------------------------------------------------------------------------------------------------- the model
class ClipModel:
    """A loaded CLIP model for the metrics: the towers on one device, the tokenizer and the caption templates."""

    def __init__(self, weights, device: Optional[str] = None, clip_model: str = "ViT-B/16", compute_dtype=torch.float16,
                 templates: Optional[Sequence[str]] = None, seed: int = 0, tokenizer=None):
        """`tokenizer`: a directory with CLIP's `vocab.json` and `merges.txt`, or an object with `encode(text) -> ids` (start and end token
        included); None: the snapshot's (ETAINV_SD_PATH/tokenizer) or, without a snapshot, the word-level stand-in, which only synthetic
        weights may be fed with (`tokenize` refuses it under any other weights)."""
        from etainv.weights import load_clip_state_dict, synthetic_clip_state_dict
        from modules.utils.tokenizer import ClipBPETokenizer, load_tokenizer
        if weights is None:
            raise ValueError("the CLIP metrics need weights=: a path, a state dict or \"synthetic\" (there is no default and no download)")
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        self.device, self.templates = str(device), list(templates) if templates is not None else ["{}"]
        if not self.templates or not all(isinstance(t, str) and "{}" in t for t in self.templates):
            raise ValueError("templates= must be a non-empty list of strings with a {} for the prompt")
        self.synthetic = isinstance(weights, str) and weights == "synthetic"
        if self.synthetic:
            if clip_model not in GEOMETRY:
                raise ValueError(f"clip_model must be one of {', '.join(GEOMETRY)} for synthetic weights, got {clip_model}")
            sd = synthetic_clip_state_dict(seed=seed, **GEOMETRY[clip_model])
        else:
            sd = load_clip_state_dict(weights)
        if self.device.startswith("cuda"):
            from etainv.nets import NativeCLIP
            with torch.cuda.device(self.device):
                self.backend = NativeCLIP(sd, compute_dtype=compute_dtype)
            self.dtype = compute_dtype
        else:
            self.backend, self.dtype = _TorchCLIP(sd), torch.float32
        self.patch, self.image = self.backend.patch, self.backend.image
        if tokenizer is None:
            self.tokenizer = load_tokenizer()
        elif isinstance(tokenizer, (str, os.PathLike)):
            files = [os.path.join(tokenizer, f) for f in ("vocab.json", "merges.txt")]
            missing = [f for f in files if not os.path.isfile(f)]
            if missing:
                raise FileNotFoundError(f"tokenizer directory {tokenizer}: {', '.join(missing)} missing (CLIP's BPE vocabulary and merges)")
            self.tokenizer = ClipBPETokenizer(*files)
        else:
            self.tokenizer = tokenizer

    def tokenize(self, texts: Sequence[str]) -> torch.Tensor:
        """(N, 77) int64: start token, the text, end token, zeros; a longer text raises, as clip.tokenize does.  Trained weights with the
        word-level stand-in tokenizer are refused: its ids lie inside CLIP's vocabulary and would score silently wrong."""
        from modules.utils.tokenizer import WordLevelTokenizer
        if not self.synthetic and isinstance(self.tokenizer, WordLevelTokenizer):
            raise ValueError("these CLIP weights are not synthetic but the only tokenizer at hand is the word-level stand-in, whose ids mean nothing to "
                             "trained weights: pass tokenizer=DIR (compute_metrics.py --clip_tokenizer DIR) with CLIP's vocab.json and merges.txt, "
                             "or set ETAINV_SD_PATH to a snapshot with a tokenizer/ directory; prompts given as token ids are taken as they are")
        rows = []
        for t in texts:
            ids = self.tokenizer.encode(t)
            if len(ids) > CONTEXT:
                raise PromptTooLong(f"Input {t} is too long for context length {CONTEXT}")
            rows.append(ids + [0] * (CONTEXT - len(ids)))
        return torch.tensor(rows, dtype=torch.int64)

    def captions(self, prompt: str) -> List[str]:
        """the prompt in every template (reference :113-115)"""
        return [t.format(prompt).replace("a a", "a").replace("the a", "a") for t in self.templates]

    def embed_images(self, x: torch.Tensor, input_range=(-1, 1)) -> torch.Tensor:
        """(N, 3, S, S) -> unit embeddings (N, P) float32 on the model's device"""
        x = x.to(self.device)
        if x.is_cuda:
            with torch.cuda.device(x.device):
                return self.backend.image_features(clip_preprocess(x, input_range, self.image, self.patch, self.dtype), x.shape[0])
        return self.backend.image_features(clip_preprocess(x, input_range, self.image, self.patch, torch.float32), x.shape[0])

    def embed_prompts(self, prompts) -> torch.Tensor:
        """B prompts (strings, or token ids (B, T, 77) / (B, 77)) -> the unit embeddings of their T captions (B, T, P) float32"""
        if torch.is_tensor(prompts):
            ids = prompts.reshape(prompts.shape[0], -1, prompts.shape[-1])
        else:
            ids = torch.stack([self.tokenize(self.captions(p)) for p in prompts])
        b, t, n = ids.shape
        if self.device.startswith("cuda"):
            with torch.cuda.device(self.device):
                e = self.backend.text_features(ids.reshape(b * t, n))
        else:
            e = self.backend.text_features(ids.reshape(b * t, n))
        return e.reshape(b, t, -1)


def _mode(name: str) -> int:
    short = name[5:] if name.startswith("clip_") else name
    if short in ("text_text", "text_text_acc"):
        raise NotImplementedError(f"clip_{short} {_BLIP}")
    if short not in MODES:
        raise ValueError(f"clip_scores computes {', '.join('clip_' + m for m in MODES)}; got {name}")
    return MODES.index(short)


def _scores_torch(mode: int, img_src, img_tgt, txt_src, txt_tgt) -> torch.Tensor:
    d = lambda t: t.double()
    pe = lambda e: (lambda m: m / m.norm(dim=-1, keepdim=True))(d(e).mean(1))
    if mode == 0:
        out = (d(img_tgt) * pe(txt_tgt)).sum(-1)
    elif mode == 1:
        out = (d(img_src) * d(img_tgt)).sum(-1)
    elif mode == 2:
        out = ((d(img_tgt) - d(img_src)) * (pe(txt_tgt) - pe(txt_src))).sum(-1)
    else:
        out = ((d(img_tgt) * pe(txt_tgt)).sum(-1) > (d(img_tgt) * pe(txt_src)).sum(-1)).double()
    return out.float()


def clip_similarity(mode: int, img_src, img_tgt, txt_src, txt_tgt) -> torch.Tensor:
    """float32 [B] scores of B pairs from their unit embeddings: img_* (B, P), txt_* (B, T, P); mode = index into MODES, or 4: all four in one
    launch, float32 [B][4] in the order of MODES"""
    if not img_tgt.is_cuda:
        if mode == 4:
            return torch.stack([_scores_torch(m, img_src, img_tgt, txt_src, txt_tgt) for m in range(4)], 1)
        return _scores_torch(mode, img_src, img_tgt, txt_src, txt_tgt)
    from etainv import _capi
    lib = _capi.load()
    c = lambda t: None if t is None else t.to(torch.float32).contiguous()
    img_src, img_tgt, txt_src, txt_tgt = c(img_src), c(img_tgt), c(txt_src), c(txt_tgt)
    b, p = img_tgt.shape
    t = txt_tgt.shape[1] if txt_tgt is not None else 1
    with torch.cuda.device(img_tgt.device):
        out = torch.empty((b, 4) if mode == 4 else (b,), dtype=torch.float32, device=img_tgt.device)
        _capi.check(lib.etainv_clip_similarity(_capi.ptr(img_src), _capi.ptr(img_tgt), _capi.ptr(txt_src), _capi.ptr(txt_tgt), b, t, p, mode,
                                               _capi.ptr(out), _capi.stream_ptr()))
    return out


def clip_scores(edit: torch.Tensor, source: torch.Tensor, source_prompts, target_prompts, which: Union[str, Sequence[str]], model: ClipModel,
                input_range=(-1, 1)) -> Dict[str, torch.Tensor]:
    """{name: float32 tensor [B]} of B pairs: `edit` the edited images, `source` the input images, both (B, 3, S, S) in `input_range`, with their
    prompts (strings, or token ids).  One preprocess launch and one image-tower pass for the 2 B images, one text-tower pass for the 2 B prompts'
    captions, one score launch (a single name: its own mode; several: the all-four mode).  Every pair is independent: row i is what a call with pair i alone returns."""
    which = (which,) if isinstance(which, str) else tuple(which)
    modes = [_mode(n) for n in which]
    if edit.shape != source.shape:
        raise ValueError(f"Input images should have the same dimensions, but got {edit.shape} and {source.shape}.")
    b = edit.shape[0]
    img = model.embed_images(torch.cat([source.to(edit.device), edit]), input_range)
    if all(m == 1 for m in modes):                                   # img_img alone: no text pass
        return {n: clip_similarity(m, img[:b], img[b:], None, None) for n, m in zip(which, modes)}
    if torch.is_tensor(source_prompts):
        prompts = torch.cat([source_prompts.reshape(b, -1, source_prompts.shape[-1]), target_prompts.reshape(b, -1, target_prompts.shape[-1])])
    else:
        if len(source_prompts) != b or len(target_prompts) != b:
            raise ValueError(f"{b} image pairs need {b} source and {b} target prompts")
        prompts = list(source_prompts) + list(target_prompts)
    txt = model.embed_prompts(prompts)
    if len(set(modes)) == 1:
        one = clip_similarity(modes[0], img[:b], img[b:], txt[:b], txt[b:])
        return {n: one for n in which}
    every = clip_similarity(4, img[:b], img[b:], txt[:b], txt[b:])
    return {n: every[:, m] for n, m in zip(which, modes)}


# ---------------------------------------------------------------------------------------------------------------- the metric classes
class CLIPSimilarity(SimpleMetric):
    """Cosine similarity of CLIP embeddings: of the edited image with the target prompt (`text_img`), of the edited image with the source image
    (`img_img`), or of the change between the two images with the change between the two prompts (`textdir_imgdir`, whose differences are not
    renormalised: it is not confined to [0, 1]).  Higher is better."""
    _mode_suffix = ""            # "_acc" in the comparison CLIPAccuracy runs

    def __init__(self, input_range: Tuple[int, int] = (-1, 1), device: Optional[str] = None, use_imagenet_templates: bool = False,
                 metric: str = "text_img", clip_model: str = "ViT-B/16", weights=None, templates: Optional[Sequence[str]] = None) -> None:
        """`metric`: "text_img", "img_img" or "textdir_imgdir" ("text_text" is refused: BLIP).  `weights`: a path, a state dict, a loaded
        `ClipModel` or "synthetic".  `templates`: the caption templates to average over; use_imagenet_templates=True requires them."""
        assert metric in ("text_img", "img_img", "text_text", "textdir_imgdir")
        super().__init__(input_range, device)
        if metric == "text_text":
            raise NotImplementedError(f"clip_text_text{self._mode_suffix} {_BLIP}")
        if use_imagenet_templates and templates is None:
            raise ValueError("use_imagenet_templates=True needs templates=: the list of caption templates is the caller's, none is shipped")
        if isinstance(weights, ClipModel):
            self.model = weights
            if templates is not None:
                raise ValueError("templates= belongs to the ClipModel that is handed over")
        else:
            self.model = ClipModel(weights, self.device, clip_model, templates=templates if use_imagenet_templates or templates is not None else None)
        self.templates = self.model.templates
        self.losses = []
        self.metric = metric

    def _which(self) -> str:
        return self.metric + self._mode_suffix

    def forward(self, source_image: Optional[torch.Tensor] = None, target_image: Optional[torch.Tensor] = None,
                source_prompt: Optional[str] = None, target_prompt: Optional[str] = None) -> torch.Tensor:
        """the metric of ONE example: images (1, 3, S, S) or (3, S, S) in `input_range`; a batch of more than one image is refused (the prompts are
        single strings: `clip_scores` is the batched call)"""
        which = self._which()
        for t in (source_image, target_image):
            if t is not None and t.dim() == 4 and t.shape[0] != 1:
                raise ValueError(f"one example per call: got a batch of {t.shape[0]} images (use clip_scores for batches)")
        need = {"text_img": (target_image, target_prompt), "img_img": (source_image, target_image),
                "textdir_imgdir": (source_image, target_image, source_prompt, target_prompt),
                "text_img_acc": (target_image, source_prompt, target_prompt)}[which]
        if any(v is None for v in need):
            raise ValueError(f"clip_{which} is missing an input it needs")
        img = lambda t: t[None] if t.dim() == 3 else t
        tgt = img(target_image)
        src = img(source_image) if source_image is not None else tgt
        tp = target_prompt if target_prompt is not None else source_prompt
        sp = source_prompt if source_prompt is not None else tp
        sp, tp = (sp, tp) if sp is not None else ("", "")
        return clip_scores(tgt, src, [sp], [tp], which, self.model, self.input_range)[which][0]

    def update(self, *args, **kwargs) -> Union[float, None]:
        try:
            return super().update(*args, **kwargs)
        except PromptTooLong as exc:            # the example could not be computed: nothing is recorded (SimpleMetric's contract for None)
            print(f"{self!r}: {exc}")
            return None

    def __repr__(self) -> str:
        return f"clip_{self.metric}"


class _CLIPComparison(CLIPSimilarity):
    """CLIPSimilarity run in the text_img_acc mode (its `repr` stays that of the similarity, as CLIPAccuracy's is built from it)"""
    _mode_suffix = "_acc"


class CLIPAccuracy(SimpleMetric):
    """The edit-success rate of pix2pix-zero (arXiv 2302.03027): an example scores 1 when the edited image's CLIP embedding is closer to the
    target prompt's than to the source prompt's, else 0 (a tie is 0); `compute` gives the fraction of examples that scored 1."""

    def __init__(self, input_range: Tuple[int, int] = (-1, 1), device: Optional[str] = None, use_imagenet_templates: bool = False,
                 metric: str = "text_img", clip_model: str = "ViT-B/16", weights=None, templates: Optional[Sequence[str]] = None) -> None:
        super().__init__(input_range, device)
        if metric != "text_img":
            raise NotImplementedError(f"clip_{metric}_acc {_BLIP}" if metric == "text_text" else f"clip_{metric}_acc is not a metric of the reference")
        self.clip_sim = _CLIPComparison(input_range, device, use_imagenet_templates, metric, clip_model, weights=weights, templates=templates)

    def forward(self, source_image: Optional[torch.Tensor] = None, target_image: Optional[torch.Tensor] = None,
                source_prompt: Optional[str] = None, target_prompt: Optional[str] = None) -> torch.Tensor:
        return self.clip_sim.forward(source_image, target_image, source_prompt, target_prompt)

    def update(self, *args, **kwargs) -> Union[float, None]:
        try:
            return super().update(*args, **kwargs)
        except PromptTooLong as exc:
            print(f"{self!r}: {exc}")
            return None

    def __repr__(self) -> str:
        return f"{self.clip_sim}_acc"
