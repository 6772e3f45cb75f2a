"""The dinovitstruct metric (reference metrics/dino_vit_structure.py:15-284): `DinoVitStructure` and `dino_structure`, the batched call it sits on.

The structure distance of Splice: the cosine self-similarity of the last block's attention keys of a DINO ViT, compared between the source image
and the edit by the mean squared difference over all n x n token pairs.  Lower is better.

Device tensors go to the HIP kernels (csrc/dino.hip and NativeDinoVision of etainv/nets.py: one preprocess launch and one tower pass for the 2 B
images, one self-similarity call).  CPU tensors, or device="cpu", go to the plain-torch float32 path below, which keeps the package and
compute_metrics.py usable without a GPU.  Both run the same steps: the range map of SimpleMetric._normalize, Resize(224) on a float tensor (torch's
antialiased bilinear interpolation, restated as per-output tables built in float64; antialias=False gives the two-tap tables of older torchvision),
the ImageNet normalisation, the tower up to `blocks[L-1].attn.qkv`, its key third, `attn_cosine_sim` (the clamp is on the product of the norms) and
the mean squared difference.

dinovitstruct_v2 is the same metric on a DINOv2 ViT (`Dinov2Model`: patch 14, LayerScale, position embeddings interpolated from the 37 x 37
table the model was trained with; reference :32-34, :120-122, :141-160): etainv_dinov2_preprocess, NativeDinov2Vision with the fused
etainv_op_layerscale_add_layernorm, and the same self-similarity call.

Weights are handed over explicitly (`weights=`: a path, a state dict, a loaded `DinoModel`, or "synthetic"); there is no default and no download.
Images must be square: DINO interpolates its position embeddings bicubically for any other shape, which is not built."""
import functools
from typing import Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from .base import SimpleMetric

MEAN = (0.485, 0.456, 0.406)          # ImageNet normalisation (reference :236)
STD = (0.229, 0.224, 0.225)
EPS = 1e-8                            # attn_cosine_sim's clamp (reference :15)
GEOMETRY = {
    "dino_vitb8": dict(width=768, layers=12, patch=8, image=224),
    "dino_vits8": dict(width=384, layers=12, patch=8, image=224),
    "dino_vitb16": dict(width=768, layers=12, patch=16, image=224),
    "dino_vits16": dict(width=384, layers=12, patch=16, image=224),
    "tiny/8": dict(width=128, layers=2, patch=8, image=32),         # synthetic weights only: quick runs
}
GEOMETRY_V2 = {
    "dinov2_vits14": dict(width=384, layers=12, patch=14, image=224, table=37),
    "dinov2_vitb14": dict(width=768, layers=12, patch=14, image=224, table=37),
    "dinov2_vitl14": dict(width=1024, layers=24, patch=14, image=224, table=37),
    "tinyv2/14": dict(width=128, layers=2, patch=14, image=42, table=5),      # synthetic weights only: 10 tokens, the table interpolated 5 -> 3
}
V2_KP = 640                           # a patch-14 row: 588 values and 52 zeros (etainv_dinov2_preprocess)


# ---------------------------------------------------------------------------------------------------------------- the resize tables
@functools.lru_cache(maxsize=32)
def resize_tables(n_in: int, n_out: int, antialias: bool = True) -> Tuple[np.ndarray, np.ndarray]:
    """(read-only, cached) (bounds [n_out][2] = (first tap, taps) int32, coef [n_out][ksize] float64 summing to 1 per row): the weights of
    F.interpolate(mode="bilinear", align_corners=False, antialias=antialias) along one axis, built in float64.  antialias=True: with
    scale = n_in / n_out, support = max(scale, 1) and c = scale (i + 0.5), the taps from max(0, int(c - support + 0.5)) up to
    min(n_in, int(c + support + 0.5)) weigh max(0, 1 - |(j + 0.5 - c) / support|), normalised.  antialias=False: the two neighbours of
    src = max(scale (i + 0.5) - 0.5, 0).  Trailing zero weights are dropped, so n_in == n_out is one tap of weight 1."""
    scale = n_in / n_out
    taps = []
    for i in range(n_out):
        if antialias:
            support = max(scale, 1.0)
            c = scale * (i + 0.5)
            first = max(0, int(c - support + 0.5))
            count = min(n_in, int(c + support + 0.5)) - first
            w = [max(0.0, 1.0 - abs((j + first - c + 0.5) / support)) for j in range(count)]
            total = 0.0
            for v in w:
                total += v
            w = [v / total for v in w]
        else:
            src = max(scale * (i + 0.5) - 0.5, 0.0)
            first = min(int(src), n_in - 1)
            lam = src - first
            w = [1.0 - lam, lam] if first + 1 < n_in else [1.0]
        while len(w) > 1 and w[-1] == 0.0:
            w.pop()
        taps.append((first, w))
    bounds = np.zeros((n_out, 2), dtype=np.int32)
    coef = np.zeros((n_out, max(len(w) for _, w in taps)), dtype=np.float64)
    for i, (first, w) in enumerate(taps):
        bounds[i] = (first, len(w))
        coef[i, :len(w)] = w
    bounds.setflags(write=False)
    coef.setflags(write=False)
    return bounds, coef


def _band_rows(bounds: np.ndarray, p: int) -> int:
    """the most input rows a band of p output rows spans"""
    first, last = bounds[0::p], bounds[p - 1::p]
    return int((last[:, 0] + last[:, 1] - first[:, 0]).max())


@functools.lru_cache(maxsize=32)
def _device_tables(n_in: int, n_out: int, p: int, antialias: bool, device: str):
    bounds, coef = resize_tables(n_in, n_out, antialias)
    return (torch.from_numpy(bounds.copy()).to(device), torch.from_numpy(coef.astype(np.float32)).to(device), coef.shape[1], _band_rows(bounds, p))


def _check_images(x: torch.Tensor, r: int, p: int) -> None:
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f"Input images should be (B, 3, H, W) tensors, but got {tuple(x.shape)}")
    if x.shape[2] != x.shape[3]:
        raise ValueError(f"dinovitstruct takes square images (DINO would interpolate its position embeddings bicubically for the others, which is "
                         f"not built), but got {tuple(x.shape[2:])}")
    if p not in (8, 16) or r % p:
        raise ValueError(f"patch size {p} must be 8 or 16 and divide the model's image size {r}")


def _range(input_range) -> Tuple[float, float]:
    lo, hi = (0.0, 1.0) if input_range is None else (float(input_range[0]), float(input_range[1]))
    if not hi > lo:
        raise ValueError(f"input_range must be (lo, hi) with hi > lo, got {input_range}")
    return lo, hi


def _resample_torch(img: torch.Tensor, bounds: np.ndarray, coef: np.ndarray) -> torch.Tensor:
    """one pass along the last axis, float32"""
    j = torch.arange(coef.shape[1])
    b = torch.from_numpy(bounds.astype(np.int64))
    idx = (b[:, :1] + j).clamp_(max=img.shape[-1] - 1)                          # [n_out][ks]; taps beyond the count carry weight 0
    return (img[..., idx] * torch.from_numpy(coef.astype(np.float32))).sum(-1)


def _patch_rows(img: torch.Tensor, p: int) -> torch.Tensor:
    b, _, r, _ = img.shape
    g = r // p
    return img.reshape(b, 3, g, p, g, p).permute(0, 2, 4, 1, 3, 5).reshape(b * g * g, 3 * p * p)


def dino_preprocess(x: torch.Tensor, input_range=(-1, 1), r: int = 224, p: int = 8, dtype=torch.float16, antialias: bool = True) -> torch.Tensor:
    """(B, 3, S, S) images in `input_range` -> the ViT's patch rows [B (r / p)^2][3 p^2] in `dtype` (element k = c p^2 + py p + px).  Device
    tensors: one etainv_dino_preprocess launch; CPU tensors: float32 torch."""
    _check_images(x, r, p)
    lo, hi = _range(input_range)
    s = x.shape[-1]
    if not x.is_cuda:
        bounds, coef = resize_tables(s, r, antialias)
        v = (x.detach().float() - lo) / (hi - lo)
        v = _resample_torch(_resample_torch(v, bounds, coef).transpose(-1, -2), bounds, coef).transpose(-1, -2)
        v = (v - torch.tensor(MEAN).view(1, 3, 1, 1)) / torch.tensor(STD).view(1, 3, 1, 1)
        return _patch_rows(v, p).contiguous().to(dtype)
    from etainv import _capi
    lib = _capi.load()
    x = x.detach().to(torch.float32).contiguous()
    b, g = x.shape[0], r // p
    tb, tc, ksize, band = _device_tables(s, r, p, bool(antialias), str(x.device))
    with torch.cuda.device(x.device):
        rows = torch.empty(b * g * g, 3 * p * p, dtype=dtype, device=x.device)
        _capi.check(lib.etainv_dino_preprocess(_capi.ptr(x), b, s, r, p, lo, hi, _capi.ptr(tb), _capi.ptr(tc), ksize, _capi.ptr(tb), _capi.ptr(tc),
                                               ksize, band, _capi.ptr(rows), _capi.dtype_code(dtype), _capi.stream_ptr()))
    return rows


def dinov2_preprocess(x: torch.Tensor, input_range=(-1, 1), r: int = 224, dtype=torch.float16, antialias: bool = True) -> torch.Tensor:
    """`dino_preprocess` for DINOv2's patch 14: (B, 3, S, S) -> patch rows [B (r / 14)^2][640] in `dtype`, element k = c 196 + py 14 + px for
    k < 588 and zero behind.  Device tensors: one etainv_dinov2_preprocess launch; CPU tensors: float32 torch."""
    _check_images_v2(x, r)
    lo, hi = _range(input_range)
    s = x.shape[-1]
    if not x.is_cuda:
        bounds, coef = resize_tables(s, r, antialias)
        v = (x.detach().float() - lo) / (hi - lo)
        v = _resample_torch(_resample_torch(v, bounds, coef).transpose(-1, -2), bounds, coef).transpose(-1, -2)
        v = (v - torch.tensor(MEAN).view(1, 3, 1, 1)) / torch.tensor(STD).view(1, 3, 1, 1)
        return F.pad(_patch_rows(v, 14), (0, V2_KP - 588)).contiguous().to(dtype)
    from etainv import _capi
    lib = _capi.load()
    x = x.detach().to(torch.float32).contiguous()
    b, g = x.shape[0], r // 14
    tb, tc, ksize, band = _device_tables(s, r, 14, bool(antialias), str(x.device))
    with torch.cuda.device(x.device):
        rows = torch.empty(b * g * g, V2_KP, dtype=dtype, device=x.device)
        _capi.check(lib.etainv_dinov2_preprocess(_capi.ptr(x), b, s, r, lo, hi, _capi.ptr(tb), _capi.ptr(tc), ksize, _capi.ptr(tb), _capi.ptr(tc), ksize,
                                                 band, _capi.ptr(rows), _capi.dtype_code(dtype), _capi.stream_ptr()))
    return rows


def _check_images_v2(x: torch.Tensor, r: int) -> None:
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f"Input images should be (B, 3, H, W) tensors, but got {tuple(x.shape)}")
    if x.shape[2] != x.shape[3]:
        raise ValueError(f"dinovitstruct_v2 takes square images (the other shapes resize to sides that are no multiples of 14, which DINOv2's own patch "
                         f"embedding refuses), but got {tuple(x.shape[2:])}")
    if r < 14 or r % 14:
        raise ValueError(f"the model's image size {r} must be a multiple of the patch size 14")


# ---------------------------------------------------------------------------------------------------------------- the float32 torch tower
class _TorchDino:
    """the tower in plain float32 torch on the CPU, over DINO's checkpoint names"""

    def __init__(self, sd: dict):
        from etainv.nets import dino_geometry
        gm = dino_geometry(sd)
        self.sd = {k: v.float() for k, v in sd.items()}
        self.d, self.patch, self.image, self.g2, self.depth = gm["width"], gm["patch"], gm["image"], gm["g2"], gm["layers"]

    def __call__(self, rows: torch.Tensor, b: int) -> torch.Tensor:
        sd, d, heads = self.sd, self.d, self.d // 64
        lin = lambda t, name: F.linear(t, sd[name + ".weight"], sd[name + ".bias"])
        ln = lambda t, name: F.layer_norm(t, (d,), sd[name + ".weight"], sd[name + ".bias"], eps=1e-6)
        pe = F.linear(rows.float(), sd["patch_embed.proj.weight"].reshape(d, -1), sd["patch_embed.proj.bias"]).reshape(b, -1, d)
        x = torch.cat([sd["cls_token"].reshape(1, 1, d).expand(b, 1, d), pe], 1) + sd["pos_embed"].reshape(1, -1, d)
        n = x.shape[1]
        sp = lambda t: t.reshape(b, n, heads, 64).transpose(1, 2)
        for i in range(self.depth):
            p = f"blocks.{i}."
            h = ln(x, p + "norm1")
            if i == self.depth - 1:
                return F.linear(h, sd[p + "attn.qkv.weight"][d:2 * d], sd[p + "attn.qkv.bias"][d:2 * d])
            q, k, v = (sp(t) for t in lin(h, p + "attn.qkv").split(d, -1))
            a = (q @ k.transpose(-1, -2) * 0.125).softmax(-1) @ v
            x = x + lin(a.transpose(1, 2).reshape(b, n, d), p + "attn.proj")
            x = x + lin(F.gelu(lin(ln(x, p + "norm2"), p + "mlp.fc1")), p + "mlp.fc2")


class _TorchDinov2:
    """the DINOv2 tower in plain float32 torch on the CPU, over the published checkpoint names"""

    def __init__(self, sd: dict, interpolate_offset: float = 0.1, image=None):
        from etainv.nets import dinov2_geometry, dinov2_position_table
        gm = dinov2_geometry(sd, image)
        self.sd = {k: v.float() for k, v in sd.items()}
        self.d, self.patch, self.image, self.g2, self.depth, self.table = gm["width"], 14, gm["image"], gm["g2"], gm["layers"], gm["table"]
        self.interpolate_offset = float(interpolate_offset)
        self.pos = dinov2_position_table(self.sd["pos_embed"], self.image // 14, self.interpolate_offset)

    def __call__(self, rows: torch.Tensor, b: int) -> torch.Tensor:
        sd, d, heads = self.sd, self.d, self.d // 64
        lin = lambda t, name: F.linear(t, sd[name + ".weight"], sd[name + ".bias"])
        ln = lambda t, name: F.layer_norm(t, (d,), sd[name + ".weight"], sd[name + ".bias"], eps=1e-6)
        pe = F.linear(rows.float()[:, :588], sd["patch_embed.proj.weight"].reshape(d, -1), sd["patch_embed.proj.bias"]).reshape(b, -1, d)
        x = torch.cat([sd["cls_token"].reshape(1, 1, d).expand(b, 1, d), pe], 1) + self.pos[None]
        n = x.shape[1]
        sp = lambda t: t.reshape(b, n, heads, 64).transpose(1, 2)
        for i in range(self.depth):
            p = f"blocks.{i}."
            h = ln(x, p + "norm1")
            if i == self.depth - 1:
                return F.linear(h, sd[p + "attn.qkv.weight"][d:2 * d], sd[p + "attn.qkv.bias"][d:2 * d])
            q, k, v = (sp(t) for t in lin(h, p + "attn.qkv").split(d, -1))
            a = (q @ k.transpose(-1, -2) * 0.125).softmax(-1) @ v
            x = x + sd[p + "ls1.gamma"] * lin(a.transpose(1, 2).reshape(b, n, d), p + "attn.proj")
            x = x + sd[p + "ls2.gamma"] * lin(F.gelu(lin(ln(x, p + "norm2"), p + "mlp.fc1")), p + "mlp.fc2")


# ---------------------------------------------------------------------------------------------------------------- the model
class DinoModel:
    """A loaded DINO ViT for the metric: the tower on one device."""

    def __init__(self, weights, device: Optional[str] = None, dino_model: str = "dino_vitb8", compute_dtype=torch.float16, antialias: bool = True,
                 seed: int = 0):
        """`weights`: a path to DINO's published checkpoint, a state dict, a loaded `DinoModel` (shared as it is), or "synthetic" (then `dino_model` picks the geometry from GEOMETRY;
        with real weights the geometry is read from the tensor shapes and `dino_model` is only the metric's printed name).  `antialias=False`
        resizes as torchvision did before it antialiased tensors."""
        from etainv.weights import load_dino_state_dict, synthetic_dino_state_dict
        if isinstance(weights, DinoModel):                            # a loaded model handed over: share its tower
            self.__dict__.update(weights.__dict__)
            return
        if weights is None:
            raise ValueError("dinovitstruct needs weights=: a path, a state dict or \"synthetic\" (there is no default and no download)")
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        if dino_model.startswith("dinov2"):
            raise NotImplementedError(f"{dino_model} is a DINOv2 model (dinovitstruct_v2): patch 14, LayerScale and interpolated position embeddings "
                                      f"are not built")
        self.device, self.name, self.antialias = str(device), dino_model, bool(antialias)
        self.synthetic = isinstance(weights, str) and weights == "synthetic"
        if self.synthetic:
            if dino_model not in GEOMETRY:
                raise ValueError(f"dino_model must be one of {', '.join(GEOMETRY)} for synthetic weights, got {dino_model}")
            sd = synthetic_dino_state_dict(seed=seed, **GEOMETRY[dino_model])
        else:
            sd = load_dino_state_dict(weights)
        if self.device.startswith("cuda"):
            from etainv.nets import NativeDinoVision
            with torch.cuda.device(self.device):
                self.backend = NativeDinoVision(sd, compute_dtype=compute_dtype)
            self.dtype = compute_dtype
        else:
            self.backend, self.dtype = _TorchDino(sd), torch.float32
        self.patch, self.image, self.width = self.backend.patch, self.backend.image, self.backend.d

    def keys(self, x: torch.Tensor, input_range=(-1, 1)) -> torch.Tensor:
        """(B, 3, S, S) -> the last block's attention keys [B][n][d], n = 1 + (image / patch)^2, in the model's dtype on its device"""
        x = x.to(self.device)
        _check_images(x, self.image, self.patch)
        if x.is_cuda:
            with torch.cuda.device(x.device):
                return self.backend(dino_preprocess(x, input_range, self.image, self.patch, self.dtype, self.antialias), x.shape[0])
        return self.backend(dino_preprocess(x, input_range, self.image, self.patch, torch.float32, self.antialias), x.shape[0])


class Dinov2Model:
    """A loaded DINOv2 ViT for dinovitstruct_v2: the surface of `DinoModel` (keys(), a loaded model is shared, "synthetic")."""

    def __init__(self, weights, device: Optional[str] = None, dino_model: str = "dinov2_vitb14", compute_dtype=torch.float16, antialias: bool = True,
                 interpolate_offset: float = 0.1, seed: int = 0, image: Optional[int] = None):
        """`weights`: a path to a published dinov2_vit{s,b,l}14 backbone checkpoint, a state dict, a loaded `Dinov2Model` (shared as it is), or
        "synthetic" (then `dino_model` picks the geometry from GEOMETRY_V2).  `interpolate_offset`: 0.1 is the published hub models' way of
        interpolating the position table (scale_factor (g + 0.1) / M); 0 is transformers' (size (g, g)).  `image`: the side the model runs at
        (None: 224, the reference's Resize; the model's own side for tables smaller than 16 x 16)."""
        from etainv.weights import load_dinov2_state_dict, synthetic_dinov2_state_dict
        if isinstance(weights, Dinov2Model):
            self.__dict__.update(weights.__dict__)
            return
        if weights is None:
            raise ValueError("dinovitstruct_v2 needs weights=: a path, a state dict or \"synthetic\" (there is no default and no download)")
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        if dino_model in ("dinov2_vitg14",) or dino_model.endswith("_reg"):
            raise NotImplementedError(f"{dino_model}: the SwiGLU feed-forward of dinov2_vitg14 and the register-token models are not built")
        self.device, self.name, self.antialias = str(device), dino_model, bool(antialias)
        self.synthetic = isinstance(weights, str) and weights == "synthetic"
        if self.synthetic:
            if dino_model not in GEOMETRY_V2:
                raise ValueError(f"dino_model must be one of {', '.join(GEOMETRY_V2)} for synthetic weights, got {dino_model}")
            sd = synthetic_dinov2_state_dict(seed=seed, **GEOMETRY_V2[dino_model])
            image = GEOMETRY_V2[dino_model]["image"] if image is None else image
        else:
            sd = load_dinov2_state_dict(weights)
        if self.device.startswith("cuda"):
            from etainv.nets import NativeDinov2Vision
            with torch.cuda.device(self.device):
                self.backend = NativeDinov2Vision(sd, compute_dtype=compute_dtype, interpolate_offset=interpolate_offset, image=image)
            self.dtype = compute_dtype
        else:
            self.backend, self.dtype = _TorchDinov2(sd, interpolate_offset, image), torch.float32
        self.patch, self.image, self.width, self.table = 14, self.backend.image, self.backend.d, self.backend.table
        self.interpolate_offset = float(interpolate_offset)

    def keys(self, x: torch.Tensor, input_range=(-1, 1)) -> torch.Tensor:
        """(B, 3, S, S) -> the last block's attention keys [B][n][d], n = 1 + (image / 14)^2, in the model's dtype on its device"""
        x = x.to(self.device)
        _check_images_v2(x, self.image)
        if x.is_cuda:
            with torch.cuda.device(x.device):
                return self.backend(dinov2_preprocess(x, input_range, self.image, self.dtype, self.antialias), x.shape[0])
        return self.backend(dinov2_preprocess(x, input_range, self.image, torch.float32, self.antialias), x.shape[0])


def key_self_similarity_mse(keys: torch.Tensor, eps: float = EPS, d: Optional[int] = None, return_norms: bool = False):
    """keys [2 B][n][ld] (rows 0 .. B-1 the sources', B .. 2B-1 the edits'; the first `d` columns of every row are used, default all) ->
    float64 [B]: the mean over all n^2 token pairs of the squared difference of the two cosine self-similarity matrices.  Device tensors: one
    etainv_dino_selfsim_mse call (the last axis must be contiguous; a row stride larger than d is passed on, not copied); CPU tensors: float64 torch."""
    if keys.dim() != 3 or keys.shape[0] % 2:
        raise ValueError(f"keys must be [2 B][n][d], got {tuple(keys.shape)}")
    b2, n, width = keys.shape
    d = width if d is None else d
    if not keys.is_cuda:
        k = keys[..., :d].double()
        norm = k.norm(dim=-1, keepdim=True)
        sim = (k @ k.transpose(-1, -2)) / (norm @ norm.transpose(-1, -2)).clamp(min=eps)
        out = (sim[b2 // 2:] - sim[:b2 // 2]).square().mean((-1, -2))
        return (out, norm[..., 0].float()) if return_norms else out
    from etainv import _capi
    lib = _capi.load()
    if keys.stride(2) != 1 or keys.stride(0) != n * keys.stride(1):
        keys = keys.contiguous()
    ld = keys.stride(1)
    with torch.cuda.device(keys.device):
        need = lib.etainv_dino_selfsim_workspace_bytes(b2 // 2, n)
        if need < 0:
            raise _capi.EtainvError(lib.etainv_last_error().decode())
        ws = torch.empty(max(need, 8) // 8 + 1, dtype=torch.float64, device=keys.device)
        out = torch.empty(b2 // 2, dtype=torch.float64, device=keys.device)
        norms = torch.empty(b2, n, dtype=torch.float32, device=keys.device) if return_norms else None
        _capi.check(lib.etainv_dino_selfsim_mse(keys.data_ptr(), b2 // 2, n, d, ld, eps, _capi.ptr(out), _capi.ptr(norms), _capi.ptr(ws),
                                                ws.numel() * 8, _capi.dtype_code(keys.dtype), _capi.stream_ptr()))
    return (out, norms) if return_norms else out


def dino_structure(edit: torch.Tensor, source: torch.Tensor, model, input_range=(-1, 1)) -> torch.Tensor:
    """float64 [B] structure distances of B pairs under `model`, a `DinoModel` (dinovitstruct) or a `Dinov2Model` (dinovitstruct_v2): `edit`
    the edited images, `source` the input images, both (B, 3, S, S) in `input_range`.  One
    preprocess launch and one tower pass for the 2 B images, one self-similarity call.  Every pair is independent: row i is what a call with
    pair i alone returns."""
    if edit.shape != source.shape:
        raise ValueError(f"Input images should have the same dimensions, but got {edit.shape} and {source.shape}.")
    keys = model.keys(torch.cat([source.to(edit.device), edit]), input_range)
    return key_self_similarity_mse(keys.contiguous())


# ---------------------------------------------------------------------------------------------------------------- the metric class
class DinoVitStructure(SimpleMetric):
    """Measure structural similarity of two images using DINO features.  Lower means better.  (Splice, arXiv 2201.00424.)"""

    def __init__(self, input_range: Tuple[int, int] = (-1, 1), device: Optional[str] = None, vit_model: Optional[str] = "dino_vitb8", weights=None,
                 antialias: bool = True) -> None:
        """`vit_model`: dino_vitb8, dino_vits8, dino_vitb16 or dino_vits16, or (dinovitstruct_v2) dinov2_vits14, dinov2_vitb14 or dinov2_vitl14.
        `weights`: a path, a state dict, a loaded `DinoModel` / `Dinov2Model` or "synthetic"."""
        super().__init__(input_range, device)
        self.vit_model = vit_model
        if isinstance(weights, (DinoModel, Dinov2Model)):
            self.model = weights
        elif vit_model.startswith("dinov2") or vit_model in GEOMETRY_V2:
            self.model = Dinov2Model(weights, self.device, vit_model, antialias=antialias)
        else:
            self.model = DinoModel(weights, self.device, vit_model, antialias=antialias)
        self.losses = []

    def forward(self, pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        """the metric of one example: `pred` the output image, `target` the ground-truth image, (1, 3, S, S) or (3, S, S) in `input_range`; a
        batch gives the SUM over its pairs, as the reference's loop does (:256-263)"""
        img = lambda t: t[None] if t.dim() == 3 else t
        rows = dino_structure(img(pred), img(target), self.model, self.input_range)
        return rows[0] if rows.shape[0] == 1 else rows.sum()

    def __repr__(self) -> str:
        return self.vit_model
