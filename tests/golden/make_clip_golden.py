"""Writes tests/golden/clip_ref.npz: a tiny randomly initialised transformers CLIPModel, its inputs, its float64 outputs and the yardstick y of
tests/test_clip_gpu.py.  Run from the repository root:  python tests/golden/make_clip_golden.py

The model: vision width 128 (2 heads), 2 layers, patch 16; text width 64, 2 layers, vocabulary 64 (start 62, end 63 = the largest id, so that
transformers' pooling and the argmax rule agree); projection 64.  Case A runs it at image size 32 (5 tokens); case B keeps layer 0 only at image
size 224 (197 tokens) with its own position embedding.  To fit the repository's size limit the matrices are stored as int8 times a power of two
(exact in fp16 and bf16) and the images as bytes.
  y = max |f_prec - f_64| over the unit embeddings, f_prec = the same model run by torch on the CPU in that dtype, f_64 in float64."""
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
from tests import clip_ref as cr  # noqa: E402

DTYPES = {"float16": torch.float16, "bfloat16": torch.bfloat16, "float32": torch.float32}


SYN_PROMPTS = ["a cat on a bench", "a photo of a red car", "dog", "a blue car in the rain"]     # tests/test_clip_gpu.py feeds the same


def build(image, layers, sd=None, text_width=64, vocab=64):
    import transformers
    enc = dict(num_hidden_layers=layers, projection_dim=64, hidden_act="quick_gelu")
    cfg = transformers.CLIPConfig(
        text_config=dict(enc, hidden_size=text_width, num_attention_heads=text_width // 64, intermediate_size=4 * text_width, vocab_size=vocab,
                         eos_token_id=vocab - 1, bos_token_id=vocab - 2, pad_token_id=0, max_position_embeddings=77, num_hidden_layers=2),
        vision_config=dict(enc, hidden_size=128, num_attention_heads=2, intermediate_size=512, patch_size=16, image_size=image), projection_dim=64)
    model = transformers.CLIPModel(cfg).eval()
    if sd is not None:
        model.load_state_dict(sd, strict=True)
    return model


def quantise(sd, g):
    """every matrix -> int8 * 2^-e with the spread of a trained layer (std about fan_in^-0.5); vectors stay fp32"""
    out, packed = {}, {}
    for k, v in sd.items():
        if not v.is_floating_point():
            continue
        if v.dim() >= 2:
            std = 0.5 if "embedding" in k and "patch" not in k else v[0].numel() ** -0.5
            e = int(round(np.log2(40.0 / std)))
            q = torch.clamp((torch.randn(v.shape, generator=g) * 40).round(), -127, 127).to(torch.int8)
            packed[k] = (q.numpy(), e)
            out[k] = q.float() * 2.0 ** -e
        elif k == "logit_scale":
            out[k] = v.detach().clone()
        else:
            if k.endswith(".weight"):                                   # (a LayerNorm's scale)
                out[k] = 1.0 + 0.1 * torch.randn(v.shape, generator=g)
            else:
                out[k] = (0.05 if k.endswith(".bias") else 0.5) * torch.randn(v.shape, generator=g)   # biases; the class embedding
            packed[k] = (out[k].numpy(), None)
    return out, packed


def pixels(u8, dtype):
    v = torch.from_numpy(u8.astype(np.float64)) / 255.0
    return ((v - torch.tensor(cr.MEAN, dtype=torch.float64).view(1, 3, 1, 1)) / torch.tensor(cr.STD, dtype=torch.float64).view(1, 3, 1, 1)).to(dtype)


def unit(model, dtype, pix=None, ids=None):
    m = model.to(dtype)
    with torch.no_grad():
        o = m.get_image_features(pixel_values=pix.to(dtype)) if pix is not None else m.get_text_features(input_ids=ids)
    o = getattr(o, "pooler_output", o)
    return (o / o.norm(dim=-1, keepdim=True)).double()


def smooth_bytes(b, s, g):
    yy, xx = torch.meshgrid(torch.linspace(0, 1, s), torch.linspace(0, 1, s), indexing="ij")
    ph = torch.rand(b, 3, 1, 1, generator=g) * 6.28
    v = 0.5 + 0.35 * torch.sin(9 * xx + ph) * torch.cos(6 * yy - 2 * ph) + 0.1 * torch.randn(b, 3, s, s, generator=g)
    return (v.clamp(0, 1) * 255).to(torch.uint8).numpy()


def main():
    g = torch.Generator().manual_seed(20240)
    torch.manual_seed(0)
    model_a = build(32, 2)
    sd_a, packed = quantise(model_a.state_dict(), g)
    model_a.load_state_dict(sd_a, strict=False)
    sd_b = {k: v for k, v in sd_a.items() if ".vision_model.encoder.layers.1." not in "." + k}
    pos_b = torch.clamp((torch.randn(197, 128, generator=g) * 40).round(), -127, 127).to(torch.int8)
    sd_b["vision_model.embeddings.position_embedding.weight"] = pos_b.float() * 2.0 ** -6
    model_b = build(224, 1)
    model_b.load_state_dict(sd_b, strict=False)
    # (strict=False: transformers keeps position_ids buffers; every parameter is checked below)
    for model, sd in ((model_a, sd_a), (model_b, sd_b)):
        have = dict(model.state_dict())
        assert all(torch.equal(have[k].float(), v.float()) for k, v in sd.items()), "a parameter was not loaded"

    img_a, img_b = smooth_bytes(8, 48, g), smooth_bytes(2, 96, g)          # A: 4 pairs (source 0-3, edit 4-7) at 48 -> 32; B: 2 images at 96 -> 224
    x = lambda u8: torch.from_numpy(u8).float() / 127.5 - 1.0               # what the tests feed: bytes as (-1, 1) floats
    res_a, res_b = cr.preprocess_u8(x(img_a), -1, 1, 32), cr.preprocess_u8(x(img_b), -1, 1, 224)

    # prompts: 4 (source, target) pairs whose text_img margin |<img_tgt, txt_tgt> - <img_tgt, txt_src>| is the largest among random candidates
    f_img_a = unit(model_a.double(), torch.float64, pix=pixels(res_a, torch.float64))
    cand = torch.zeros(64, 77, dtype=torch.int64)
    for i in range(64):
        n = 2 + i % 9
        cand[i, 0], cand[i, 1:1 + n], cand[i, 1 + n] = 62, torch.randint(1, 62, (n,), generator=g), 63
    f_cand = unit(model_a.double(), torch.float64, ids=cand)
    ids = torch.zeros(8, 77, dtype=torch.int64)                              # rows 0-3 source prompts, 4-7 target prompts
    used = set()
    for pair in range(4):
        sim = f_cand @ f_img_a[4 + pair]
        order = [int(i) for i in sim.argsort() if int(i) not in used]
        lo_i, hi_i = order[0], order[-1]
        used |= {lo_i, hi_i}
        src, tgt = (lo_i, hi_i) if pair % 2 == 0 else (hi_i, lo_i)           # pairs 0, 2: acc = 1; pairs 1, 3: acc = 0
        ids[pair], ids[4 + pair] = cand[src], cand[tgt]

    out = {"img_a_u8": img_a, "img_b_u8": img_b, "ids": ids.numpy().astype(np.int16)}
    f64 = {"img_a": f_img_a, "img_b": unit(model_b.double(), torch.float64, pix=pixels(res_b, torch.float64)),
           "txt": unit(model_a.double(), torch.float64, ids=ids)}
    # the float64 restatement agrees with transformers on this model (tests/test_clip_ref.py pins it on another)
    assert (cr.image_features(sd_a, cr.patch_rows(res_a, 16), 8) - f64["img_a"]).abs().max() < 1e-12
    assert (cr.image_features(sd_b, cr.patch_rows(res_b, 16), 2) - f64["img_b"]).abs().max() < 1e-12
    assert (cr.text_features(sd_a, ids) - f64["txt"]).abs().max() < 1e-12
    for k, v in f64.items():
        out["f64_" + k] = v.numpy()
    for name, dt in DTYPES.items():
        for k, (model, sd, pix, tok) in {"img_a": (model_a, sd_a, res_a, None), "img_b": (model_b, sd_b, res_b, None),
                                         "txt": (model_a, sd_a, None, ids)}.items():
            m = build(32 if model is model_a else 224, 2 if model is model_a else 1)
            m.load_state_dict(sd, strict=False)
            f = unit(m, dt, pix=None if pix is None else pixels(pix, dt), ids=tok)
            out[f"y_{k}_{name}"] = np.float64((f - f64[k]).abs().max().item())
            print(f"y {k} {name}: {out[f'y_{k}_{name}']:.3e}")
    # the library's synthetic weights at the tiny geometry (EditMetric(..., clip_weights="synthetic", clip_model="tiny/16")): y for them too
    sys.path.insert(0, str(ROOT / "eta-inversion_amd"))
    from etainv.weights import synthetic_clip_state_dict
    from metrics.clip_similarity import GEOMETRY
    from modules.utils.tokenizer import WordLevelTokenizer
    sd_s = synthetic_clip_state_dict(**GEOMETRY["tiny/16"])
    tok = WordLevelTokenizer()
    ids_s = torch.tensor([(lambda t: t + [0] * (77 - len(t)))(tok.encode(p)) for p in SYN_PROMPTS])
    syn = lambda: (lambda m: (m.load_state_dict(sd_s, strict=False), m)[1])(build(32, 2, text_width=128, vocab=49408))
    assert all(torch.equal(dict(syn().state_dict())[k], v) for k, v in sd_s.items())
    f64_s = {"syn_img": unit(syn().double(), torch.float64, pix=pixels(res_a, torch.float64)), "syn_txt": unit(syn().double(), torch.float64, ids=ids_s)}
    assert (cr.image_features(sd_s, cr.patch_rows(res_a, 16), 8) - f64_s["syn_img"]).abs().max() < 1e-12
    assert (cr.text_features(sd_s, ids_s) - f64_s["syn_txt"]).abs().max() < 1e-12
    for k, v in f64_s.items():
        out["f64_" + k] = v.numpy()
    for name, dt in DTYPES.items():
        for k, kw in (("syn_img", dict(pix=pixels(res_a, dt))), ("syn_txt", dict(ids=ids_s))):
            out[f"y_{k}_{name}"] = np.float64((unit(syn(), dt, **kw) - f64_s[k]).abs().max().item())
            print(f"y {k} {name}: {out[f'y_{k}_{name}']:.3e}")
    margin = (f64["txt"][4:] * f64["img_a"][4:]).sum(-1) - (f64["txt"][:4] * f64["img_a"][4:]).sum(-1)
    print("text_img margins of the four pairs:", margin.tolist())
    for k, (arr, e) in packed.items():
        out["w:" + k] = arr
        if e is not None:
            out["e:" + k] = np.int8(e)
    out["w:pos_b"], out["e:pos_b"] = pos_b.numpy(), np.int8(6)
    path = ROOT / "tests" / "golden" / "clip_ref.npz"
    np.savez_compressed(path, **out)
    print(f"{path}: {path.stat().st_size / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
