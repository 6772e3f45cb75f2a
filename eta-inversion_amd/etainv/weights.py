"""UNet weights for the engine: deterministic synthetic SD1.x-shaped parameters (no network / no checkpoint in the
build image) or a local diffusers snapshot (`unet/diffusion_pytorch_model.safetensors`)."""
import math
import zlib
from pathlib import Path

import torch

_RES_OUT = ("conv2.weight", ".to_out.", ".ff.net.2.", ".proj_out.")


_memo = None          # process-level memo of the synthetic tensors (3.4 GB of host memory for the UNet): off unless asked for


def memoize_synthetic(on: bool = True):
    """Keep every synthetic tensor generated from now on in host memory, so that a process which builds several engines (the test suite,
    A/B benchmarks) pays the 860 M single-threaded `randn` draws once.  Callers must not modify the returned tensors."""
    global _memo
    _memo = {} if on else None


def synthetic_tensor(name: str, shape, seed: int = 0) -> torch.Tensor:
    """Synthetic value of one parameter, a pure function of (name, shape, seed):
    norm scales 1 + 0.1 N(0,1); biases 0.05 N(0,1); matrices / kernels N(0,1)/sqrt(fan_in), halved on the
    residual-branch output layers so the random network stays well inside fp16 range."""
    if _memo is not None:
        key = (name, tuple(int(s) for s in shape), seed)
        if key not in _memo:
            _memo[key] = _synthetic_tensor(name, shape, seed)
        return _memo[key]
    return _synthetic_tensor(name, shape, seed)


def _synthetic_tensor(name, shape, seed):
    g = torch.Generator().manual_seed((zlib.crc32(name.encode()) + 1000003 * seed) & 0x7FFFFFFF)
    shape = tuple(int(s) for s in shape)
    if len(shape) == 1:
        base = torch.randn(shape, generator=g)
        return 1.0 + 0.1 * base if name.endswith(".weight") else 0.05 * base
    fan_in = math.prod(shape[1:])
    gain = 0.5 if (name.endswith(_RES_OUT[0]) or any(k in name for k in _RES_OUT[1:])) else 1.0
    return torch.randn(shape, generator=g) * (gain / math.sqrt(fan_in))


def load_snapshot(path) -> dict:
    """state dict of `<path>/unet/diffusion_pytorch_model(.fp16).safetensors` (diffusers layout)."""
    from safetensors.torch import load_file
    root = Path(path)
    for cand in ("unet/diffusion_pytorch_model.safetensors", "unet/diffusion_pytorch_model.fp16.safetensors",
                 "diffusion_pytorch_model.safetensors"):
        if (root / cand).exists():
            return {k: v.float() for k, v in load_file(str(root / cand)).items()}
    raise FileNotFoundError(f"no UNet safetensors under {root}")


_OLD_VAE_ATTN = {"query": "to_q", "key": "to_k", "value": "to_v", "proj_attn": "to_out.0"}


def load_component(path, sub) -> dict:
    """state dict of `<path>/<sub>/*.safetensors` for sub in {"vae", "text_encoder"}; pre-0.18 diffusers VAE attention
    names (query/key/value/proj_attn) are mapped to to_q/to_k/to_v/to_out.0."""
    from safetensors.torch import load_file
    root = Path(path) / sub
    for cand in ("diffusion_pytorch_model.safetensors", "diffusion_pytorch_model.fp16.safetensors", "model.safetensors", "model.fp16.safetensors"):
        if (root / cand).exists():
            sd = {}
            for k, v in load_file(str(root / cand)).items():
                parts = k.split(".")
                if sub == "vae" and "attentions" in parts:
                    k = ".".join(parts[:-2] + [_OLD_VAE_ATTN.get(parts[-2], parts[-2]), parts[-1]]) if parts[-2] in _OLD_VAE_ATTN else k
                v = v.float()
                if sub == "vae" and v.dim() == 4 and ".attentions." in k:     # old checkpoints keep 1x1 convs for q/k/v/out
                    v = v.reshape(v.shape[0], v.shape[1])
                sd[k] = v
            return sd
    raise FileNotFoundError(f"no safetensors under {root}")


# ---- CLIP (the metrics' model): transformers `CLIPModel` state-dict names throughout
def synthetic_clip_tensor(name: str, shape, seed: int = 0) -> torch.Tensor:
    """Synthetic value of one CLIP parameter: token / position / class embeddings 0.5 N(0, 1) (the rule of NativeCLIPText), everything else
    `synthetic_tensor`"""
    if "embedding" in name and "patch_embedding" not in name:
        g = torch.Generator().manual_seed((zlib.crc32(name.encode()) + 1000003 * seed) & 0x7FFFFFFF)
        return 0.5 * torch.randn(tuple(int(s) for s in shape), generator=g)
    return synthetic_tensor("clip." + name, shape, seed)


def synthetic_clip_state_dict(width=768, layers=12, patch=16, image=224, proj=512, text_width=512, text_layers=12, vocab=49408, seed=0) -> dict:
    """every parameter the CLIP towers read, synthetic: what NativeCLIP builds without a state dict, as a state dict (the CPU path of the metrics
    runs on the same values)"""
    shapes = {"vision_model.embeddings.class_embedding": (width,),
              "vision_model.embeddings.patch_embedding.weight": (width, 3, patch, patch),
              "vision_model.embeddings.position_embedding.weight": ((image // patch) ** 2 + 1, width),
              "text_model.embeddings.token_embedding.weight": (vocab, text_width),
              "text_model.embeddings.position_embedding.weight": (77, text_width),
              "visual_projection.weight": (proj, width), "text_projection.weight": (proj, text_width)}
    for ln, d in (("vision_model.pre_layrnorm", width), ("vision_model.post_layernorm", width), ("text_model.final_layer_norm", text_width)):
        shapes[ln + ".weight"] = shapes[ln + ".bias"] = (d,)
    for pre, d, n in (("vision_model.", width, layers), ("text_model.", text_width, text_layers)):
        for i in range(n):
            p = f"{pre}encoder.layers.{i}."
            for lin, (o, k) in {"self_attn.q_proj": (d, d), "self_attn.k_proj": (d, d), "self_attn.v_proj": (d, d), "self_attn.out_proj": (d, d),
                                "mlp.fc1": (4 * d, d), "mlp.fc2": (d, 4 * d)}.items():
                shapes[p + lin + ".weight"], shapes[p + lin + ".bias"] = (o, k), (o,)
            for ln in ("layer_norm1", "layer_norm2"):
                shapes[p + ln + ".weight"] = shapes[p + ln + ".bias"] = (d,)
    return {name: synthetic_clip_tensor(name, shape, seed) for name, shape in shapes.items()}


_OPENAI_BLOCK = {"ln_1": "layer_norm1", "ln_2": "layer_norm2", "attn.out_proj": "self_attn.out_proj", "mlp.c_fc": "mlp.fc1", "mlp.c_proj": "mlp.fc2"}
_OPENAI_TOP = {"visual.conv1.weight": "vision_model.embeddings.patch_embedding.weight",
               "visual.class_embedding": "vision_model.embeddings.class_embedding",
               "visual.positional_embedding": "vision_model.embeddings.position_embedding.weight",
               "visual.ln_pre.weight": "vision_model.pre_layrnorm.weight", "visual.ln_pre.bias": "vision_model.pre_layrnorm.bias",
               "visual.ln_post.weight": "vision_model.post_layernorm.weight", "visual.ln_post.bias": "vision_model.post_layernorm.bias",
               "token_embedding.weight": "text_model.embeddings.token_embedding.weight",
               "positional_embedding": "text_model.embeddings.position_embedding.weight",
               "ln_final.weight": "text_model.final_layer_norm.weight", "ln_final.bias": "text_model.final_layer_norm.bias",
               "logit_scale": "logit_scale"}


def openai_clip_to_transformers(sd: dict) -> dict:
    """An OpenAI `clip` state dict under transformers' `CLIPModel` names: `attn.in_proj_*` split into q / k / v, the embeddings and norms
    renamed, `visual.proj` and `text_projection` transposed (OpenAI multiplies from the right)."""
    out = {}
    for k, v in sd.items():
        v = v.detach()
        if k in _OPENAI_TOP:
            out[_OPENAI_TOP[k]] = v
        elif k == "visual.proj":
            out["visual_projection.weight"] = v.t().contiguous()
        elif k == "text_projection":
            out["text_projection.weight"] = v.t().contiguous()
        elif ".resblocks." in k:
            head, rest = k.split(".resblocks.")
            n, rest = rest.split(".", 1)
            p = ("vision_model." if head == "visual.transformer" else "text_model.") + f"encoder.layers.{n}."
            if rest.startswith("attn.in_proj_"):
                kind = rest[len("attn.in_proj_"):]
                for name, part in zip(("q_proj", "k_proj", "v_proj"), v.chunk(3, dim=0)):
                    out[p + f"self_attn.{name}.{kind}"] = part.contiguous()
            else:
                mod, kind = rest.rsplit(".", 1)
                out[p + _OPENAI_BLOCK[mod] + "." + kind] = v
        elif k in ("input_resolution", "context_length", "vocab_size"):
            continue                                                   # sizes the TorchScript archive carries as tensors
        else:
            raise KeyError(f"unexpected key in an OpenAI CLIP state dict: {k}")
    return out


def load_clip_state_dict(path) -> dict:
    """The CLIP state dict at `path` (or the dict given) under transformers' `CLIPModel` names, fp32.  Accepted: a transformers `CLIPModel`
    state dict (.safetensors or a torch file) and an OpenAI `clip` checkpoint -- the TorchScript archive `clip.load` caches or a plain state
    dict -- which is renamed.  The geometry is read from the tensor shapes (nets.clip_geometry)."""
    if isinstance(path, dict):
        sd = path
    elif str(path).endswith(".safetensors"):
        from safetensors.torch import load_file
        sd = load_file(str(path))
    else:
        try:
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", DeprecationWarning)      # (the archive `clip.load` caches IS TorchScript)
                sd = torch.jit.load(str(path), map_location="cpu").state_dict()
        except RuntimeError:
            sd = torch.load(str(path), map_location="cpu", weights_only=True)
        if "state_dict" in sd:
            sd = sd["state_dict"]
    if "visual.conv1.weight" in sd:
        sd = openai_clip_to_transformers(sd)
    if "vision_model.embeddings.patch_embedding.weight" not in sd or "text_projection.weight" not in sd:
        raise ValueError("not a CLIP state dict with a ViT image tower: vision_model.embeddings.patch_embedding.weight / text_projection.weight missing")
    return {k: v.float() for k, v in sd.items() if torch.is_tensor(v) and v.is_floating_point()}


# ---- DINO (the dinovitstruct metric's model): the names of DINO's published ViT checkpoints throughout
_DINO_V2_KEYS = ("ls1", "ls2", "gamma_1", "gamma_2", "register_tokens", "mask_token")


def synthetic_dino_state_dict(width=768, layers=12, patch=8, image=224, seed=0) -> dict:
    """every parameter the DINO tower reads, synthetic: class token and position embeddings 0.5 N(0, 1), everything else `synthetic_tensor`"""
    d = width
    shapes = {"cls_token": (1, 1, d), "pos_embed": (1, (image // patch) ** 2 + 1, d), "patch_embed.proj.weight": (d, 3, patch, patch),
              "patch_embed.proj.bias": (d,), "norm.weight": (d,), "norm.bias": (d,)}
    for i in range(layers):
        p = f"blocks.{i}."
        for lin, (o, k) in {"attn.qkv": (3 * d, d), "attn.proj": (d, d), "mlp.fc1": (4 * d, d), "mlp.fc2": (d, 4 * d)}.items():
            shapes[p + lin + ".weight"], shapes[p + lin + ".bias"] = (o, k), (o,)
        for ln in ("norm1", "norm2"):
            shapes[p + ln + ".weight"] = shapes[p + ln + ".bias"] = (d,)
    out = {}
    for name, shape in shapes.items():
        if name in ("cls_token", "pos_embed"):
            g = torch.Generator().manual_seed((zlib.crc32(("dino." + name).encode()) + 1000003 * seed) & 0x7FFFFFFF)
            out[name] = 0.5 * torch.randn(shape, generator=g)
        else:
            out[name] = synthetic_tensor("dino." + name, shape, seed)
    return out


def load_dino_state_dict(path) -> dict:
    """The DINO ViT state dict at `path` (or the dict given), fp32, under the names of DINO's published backbone checkpoints (`cls_token`,
    `pos_embed`, `patch_embed.proj`, `blocks.N.*`).  A full training checkpoint is unwrapped (`teacher`, else `state_dict`) and the prefixes
    `module.` and `backbone.` are stripped; the projection head's tensors are dropped.  DINOv2 state dicts (LayerScale, register tokens) are
    refused: that model is `dinovitstruct_v2`'s (`load_dinov2_state_dict`)."""
    sd = path if isinstance(path, dict) else torch.load(str(path), map_location="cpu", weights_only=True)
    for wrap in ("teacher", "state_dict"):
        if wrap in sd and isinstance(sd[wrap], dict):
            sd = sd[wrap]
            break
    out = {}
    for k, v in sd.items():
        for pre in ("module.", "backbone."):
            if k.startswith(pre):
                k = k[len(pre):]
        if k.startswith("head.") or not torch.is_tensor(v) or not v.is_floating_point():
            continue
        out[k] = v.detach().float()
    bad = sorted({part for k in out for part in k.split(".") if part in _DINO_V2_KEYS})
    if bad:
        raise ValueError(f"a DINOv2 state dict ({', '.join(bad)}): dinovitstruct takes the DINO ViT checkpoints; dinovitstruct_v2 (patch 14, LayerScale, "
                         f"interpolated position embeddings) is not built here: load_dinov2_state_dict")
    missing = [k for k in ("cls_token", "pos_embed", "patch_embed.proj.weight", "patch_embed.proj.bias", "blocks.0.attn.qkv.weight") if k not in out]
    if missing:
        raise ValueError(f"not a DINO ViT state dict: {', '.join(missing)} missing")
    return out


# ---- DINOv2 (the dinovitstruct_v2 metric's model): the names of the published dinov2_vit{s,b,l}14 backbone checkpoints
def synthetic_dinov2_state_dict(width=768, layers=12, patch=14, image=224, table=37, seed=0) -> dict:
    """every parameter the DINOv2 tower reads, synthetic: the DINO recipe (class token and position embeddings 0.5 N(0, 1), everything else
    `synthetic_tensor`) over a position table of `table` x `table` patches, plus the LayerScale vectors `blocks.N.ls{1,2}.gamma`: magnitudes
    log-uniform in [1e-5, 1] (DINOv2 initialises them at 1e-5 and trained values span that range), random sign.  `image` is where the model
    runs (dinov2_geometry); it does not shape any tensor."""
    del image
    d = width
    shapes = {"cls_token": (1, 1, d), "pos_embed": (1, table * table + 1, d), "patch_embed.proj.weight": (d, 3, patch, patch),
              "patch_embed.proj.bias": (d,), "norm.weight": (d,), "norm.bias": (d,), "mask_token": (1, d)}
    for i in range(layers):
        p = f"blocks.{i}."
        for lin, (o, k) in {"attn.qkv": (3 * d, d), "attn.proj": (d, d), "mlp.fc1": (4 * d, d), "mlp.fc2": (d, 4 * d)}.items():
            shapes[p + lin + ".weight"], shapes[p + lin + ".bias"] = (o, k), (o,)
        for ln in ("norm1", "norm2"):
            shapes[p + ln + ".weight"] = shapes[p + ln + ".bias"] = (d,)
        shapes[p + "ls1.gamma"] = shapes[p + "ls2.gamma"] = (d,)
    out = {}
    for name, shape in shapes.items():
        g = torch.Generator().manual_seed((zlib.crc32(("dinov2." + name).encode()) + 1000003 * seed) & 0x7FFFFFFF)
        if name in ("cls_token", "pos_embed"):
            out[name] = 0.5 * torch.randn(shape, generator=g)
        elif name.endswith(".gamma"):
            sign = torch.randint(0, 2, shape, generator=g).float() * 2 - 1
            out[name] = sign * torch.pow(10.0, -5.0 * torch.rand(shape, generator=g))
        elif name == "mask_token":
            out[name] = torch.zeros(shape)
        else:
            out[name] = synthetic_tensor("dinov2." + name, shape, seed)
    return out


def load_dinov2_state_dict(path) -> dict:
    """The DINOv2 ViT state dict at `path` (or the dict given), fp32, under the names of the published backbone checkpoints (`cls_token`,
    `pos_embed`, `patch_embed.proj`, `blocks.N.{norm1, attn, ls1, norm2, mlp, ls2}`).  Unwrapped and stripped as `load_dino_state_dict` does;
    `head.*` is dropped.  Required: `blocks.0.ls1.gamma` (a DINO checkpoint goes to `load_dino_state_dict`).  Refused, with the reason: the
    register-token models (`register_tokens`) and dinov2_vitg14 (SwiGLU: `mlp.w12`)."""
    sd = path if isinstance(path, dict) else torch.load(str(path), map_location="cpu", weights_only=True)
    for wrap in ("teacher", "state_dict"):
        if wrap in sd and isinstance(sd[wrap], dict):
            sd = sd[wrap]
            break
    out = {}
    for k, v in sd.items():
        for pre in ("module.", "backbone."):
            if k.startswith(pre):
                k = k[len(pre):]
        if k.startswith("head.") or not torch.is_tensor(v) or not v.is_floating_point():
            continue
        out[k] = v.detach().float()
    if "register_tokens" in out:
        raise ValueError("a DINOv2 state dict with register_tokens: the register-token models (dinov2_vit*14_reg) are not built (they also "
                         "interpolate their position embeddings with antialiasing and without the 0.1 offset)")
    if any(".mlp.w12." in k or ".mlp.w3." in k for k in out):
        raise ValueError("a DINOv2 state dict with mlp.w12 / mlp.w3: dinov2_vitg14's SwiGLU feed-forward is not built (vits14, vitb14 and vitl14 are)")
    missing = [k for k in ("cls_token", "pos_embed", "patch_embed.proj.weight", "patch_embed.proj.bias", "blocks.0.attn.qkv.weight", "blocks.0.ls1.gamma")
               if k not in out]
    if missing:
        raise ValueError(f"not a DINOv2 ViT state dict: {', '.join(missing)} missing (a DINO checkpoint without LayerScale is dinovitstruct's: "
                         f"load_dino_state_dict)")
    return out


# ---- LPIPS (the lpips / bglpips metrics' model): torchvision's AlexNet `features` and the five 1x1 `lin` heads of lpips.LPIPS(net='alex')
LPIPS_CONVS = (0, 3, 6, 8, 10)                                      # positions of the five convolutions in torchvision's `features`
LPIPS_KERNELS = ((11, 4, 2), (5, 1, 2), (3, 1, 1), (3, 1, 1), (3, 1, 1))   # (kernel, stride, pad) per convolution
LPIPS_WIDTHS = {"alex": (64, 192, 384, 256, 256), "tiny": (16, 32, 48, 32, 32)}   # "tiny": synthetic weights only, quick CPU runs
LPIPS_SHIFT, LPIPS_SCALE = (-.030, -.088, -.188), (.458, .448, .450)


def lpips_shapes(widths) -> dict:
    """name -> shape of every tensor the LPIPS tower reads, under the loader's own names: features.N.{weight, bias}, lin{i}.model.1.weight"""
    shapes, cin = {}, 3
    for i, (n, c) in enumerate(zip(LPIPS_CONVS, widths)):
        k = LPIPS_KERNELS[i][0]
        shapes[f"features.{n}.weight"], shapes[f"features.{n}.bias"], shapes[f"lin{i}.model.1.weight"] = (c, cin, k, k), (c,), (1, c, 1, 1)
        cin = c
    return shapes


def synthetic_lpips_state_dict(seed=0, net="alex") -> dict:
    """every parameter the LPIPS tower reads, synthetic: He-scaled convolutions N(0, 2 / fan_in) so that activations stay O(1) through the
    five ReLUs, biases 0.05 N(0, 1) (both signs), `lin` weights U(0, 4 / C) (non-negative, of order 1 / C, as the trained heads are)"""
    if net not in LPIPS_WIDTHS:
        raise ValueError(f"lpips net must be one of {', '.join(LPIPS_WIDTHS)}, got {net}")
    out = {}
    for name, shape in lpips_shapes(LPIPS_WIDTHS[net]).items():
        g = torch.Generator().manual_seed((zlib.crc32(("lpips." + net + "." + name).encode()) + 1000003 * seed) & 0x7FFFFFFF)
        if name.startswith("lin"):
            out[name] = torch.rand(shape, generator=g) * (4.0 / shape[1])
        elif name.endswith(".bias"):
            out[name] = 0.05 * torch.randn(shape, generator=g)
        else:
            out[name] = torch.randn(shape, generator=g) * math.sqrt(2.0 / (shape[1] * shape[2] * shape[3]))
    return out


def load_lpips_state_dict(weights) -> dict:
    """The LPIPS (v0.1, AlexNet) parameters at `weights`, fp32, under the names of `lpips_shapes`.  Accepted: a path or a dict in the form of
    lpips.LPIPS(net='alex').state_dict() (`net.slice{1..5}.{0,3,6,8,10}.{weight,bias}`, and `lin{i}.model.1.weight` or
    `lins.{i}.model.1.weight`); torchvision's AlexNet names (`features.{0,3,6,8,10}.*`) together with the `lin{i}` keys; or a pair
    (backbone, linear heads) of paths or dicts, merged.  Keys are matched by their suffix, so any prefix (`module.`, `net.`) is taken.  A
    `scaling_layer.shift` / `.scale` in the file must equal LPIPS's constants: the kernels hold them.  Shapes are checked, and a refusal
    names the missing key.  NOT VERIFIED against a trained file: neither the lpips package nor torchvision's checkpoint was at hand when this
    was written, and the key names above are restated from memory."""
    import re
    parts = weights if isinstance(weights, (tuple, list)) else [weights]
    merged = {}
    for part in parts:
        sd = part if isinstance(part, dict) else torch.load(str(part), map_location="cpu", weights_only=True)
        if "state_dict" in sd and isinstance(sd["state_dict"], dict):
            sd = sd["state_dict"]
        merged.update({k: v for k, v in sd.items() if torch.is_tensor(v)})
    out = {}
    conv = re.compile(r"(^|\.)(features|slice[1-5])\.(0|3|6|8|10)\.(weight|bias)$")
    lin = re.compile(r"(^|\.)lins?\.?([0-4])\.model\.1\.weight$")
    for k, v in merged.items():
        m = conv.search(k)
        if m:
            out[f"features.{m.group(3)}.{m.group(4)}"] = v.detach().float()
            continue
        m = lin.search(k)
        if m:
            out[f"lin{m.group(2)}.model.1.weight"] = v.detach().float().reshape(1, -1, 1, 1)
            continue
        for name, want in (("shift", LPIPS_SHIFT), ("scale", LPIPS_SCALE)):
            if k.endswith("scaling_layer." + name) and not torch.allclose(v.detach().float().flatten(), torch.tensor(want), rtol=0, atol=1e-6):
                raise ValueError(f"LPIPS state dict: {k} is {v.flatten().tolist()}, but the kernels hold {want}")
    if "features.0.weight" not in out and "lin0.model.1.weight" not in out:
        raise ValueError("not an LPIPS state dict: neither features.0.weight (net.slice1.0.weight) nor lin0.model.1.weight found")
    widths = [out[f"features.{n}.weight"].shape[0] if f"features.{n}.weight" in out else 0 for n in LPIPS_CONVS]
    for name, shape in lpips_shapes(widths).items():
        if name not in out:
            raise ValueError(f"LPIPS state dict: {name} missing")
        if tuple(out[name].shape) != tuple(shape):
            raise ValueError(f"LPIPS state dict: {name} has shape {tuple(out[name].shape)}, expected {tuple(shape)}")
    return out
