"""Pins tests/dino_ref.py without a GPU: the resize against F.interpolate, the tower's keys against transformers' ViTModel, the self-similarity and
the score against what the reference's own `attn_cosine_sim`, `F.mse_loss` and `DinoVitStructure` gave (recorded in tests/golden/dino_ref.npz by
tests/golden/make_dino_golden.py), and the fixture's float64 keys and scores against dino_ref as it stands."""
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import dino_ref as dr

GOLDEN = Path(__file__).resolve().parent / "golden"


@pytest.fixture(scope="module")
def z():
    return np.load(GOLDEN / "dino_ref.npz")


@pytest.mark.parametrize("antialias", [True, False])
@pytest.mark.parametrize("s,r", [(64, 224), (100, 224), (224, 224), (300, 224), (512, 224), (20, 32)])
def test_resize_is_torchs_bilinear_interpolation(s, r, antialias):
    x = torch.rand(2, 3, s, s, dtype=torch.float64, generator=torch.Generator().manual_seed(s))
    want = F.interpolate(x, size=(r, r), mode="bilinear", align_corners=False, antialias=antialias)
    got = dr.resize(x, r, antialias)
    err = (got - want).abs().max().item()
    bounds, coef = dr.resize_tables(s, r, antialias)
    print(f"dino-resize {s}->{r} antialias={antialias}: max |diff| {err:.3e}, {coef.shape[1]} taps")
    assert got.shape == want.shape and err <= 1e-12
    assert np.allclose(coef.sum(1), 1.0, atol=1e-15) and (coef >= 0).all()
    if antialias:
        assert coef.shape[1] == {64: 2, 100: 2, 224: 1, 300: 3, 512: 5, 20: 2}[s]
    else:
        assert coef.shape[1] == (1 if s == r else 2)
    if s == r:
        assert torch.equal(got, x)


# transformers' ViTModel names -> DINO's
def _to_dino_names(sd, layers):
    d = sd["embeddings.cls_token"].shape[-1]
    out = {"cls_token": sd["embeddings.cls_token"], "pos_embed": sd["embeddings.position_embeddings"],
           "patch_embed.proj.weight": sd["embeddings.patch_embeddings.projection.weight"],
           "patch_embed.proj.bias": sd["embeddings.patch_embeddings.projection.bias"]}
    for i in range(layers):
        s, p = f"layers.{i}.", f"blocks.{i}."
        for kind in ("weight", "bias"):
            out[p + f"attn.qkv.{kind}"] = torch.cat([sd[s + f"attention.{n}_proj.{kind}"] for n in ("q", "k", "v")])
            out[p + f"attn.proj.{kind}"] = sd[s + f"attention.o_proj.{kind}"]
            out[p + f"norm1.{kind}"], out[p + f"norm2.{kind}"] = sd[s + f"layernorm_before.{kind}"], sd[s + f"layernorm_after.{kind}"]
            out[p + f"mlp.fc1.{kind}"], out[p + f"mlp.fc2.{kind}"] = sd[s + f"mlp.fc1.{kind}"], sd[s + f"mlp.fc2.{kind}"]
    assert out["blocks.0.attn.qkv.weight"].shape == (3 * d, d)
    return out


def test_keys_are_those_of_transformers_vit():
    import transformers
    torch.manual_seed(3)
    cfg = transformers.ViTConfig(hidden_size=128, num_hidden_layers=3, num_attention_heads=2, intermediate_size=512, image_size=32, patch_size=8,
                                 layer_norm_eps=1e-6, hidden_act="gelu")
    model = transformers.ViTModel(cfg, add_pooling_layer=False).double().eval()
    with torch.no_grad():                                             # the fresh model's biases and class token are zero: make every term count
        for name, p in model.named_parameters():
            if p.dim() == 1 or "cls_token" in name or "position" in name:
                p.add_(0.1 * torch.randn(p.shape, dtype=p.dtype))
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    names = _to_dino_names(sd, 3)
    src, edit = dr.make_images(2, 48, -1, 1, seed=5)
    pix = dr.preprocess(torch.cat([src, edit]), -1, 1, 32)
    taken = []
    hook = model.layers[-1].attention.k_proj.register_forward_hook(lambda mod, inp, out: taken.append(out.detach()))
    with torch.no_grad():
        model(pixel_values=pix)
    hook.remove()
    got = dr.keys(names, dr.patch_rows(pix, 8), 4)
    err = (got - taken[0]).abs().max().item()
    print(f"dino-ref keys against transformers ViTModel: max |diff| {err:.3e} (|K| max {taken[0].abs().max():.2f})")
    assert got.shape == taken[0].shape == (4, 17, 128) and err <= 1e-10
    assert dr.geometry(names) == {"width": 128, "patch": 8, "image": 32, "layers": 3}


def test_self_similarity_and_score_are_the_references(z):
    sd, x, b = dr.case_inputs("a20")
    k = dr.image_keys(sd, x, -1, 1)
    row = int(z["ref_zero_row"])
    zero = k[[0, 8]].clone()
    zero[0, row] = 0.0
    src, edit = torch.cat([k[:8], zero[:1]]), torch.cat([k[8:], zero[1:]])
    sims, mse = torch.from_numpy(z["ref_sim"]), torch.from_numpy(z["ref_mse"])
    assert sims.shape == (9, 2, 17, 17) and mse.shape == (9,)
    assert (dr.self_sim(src) - sims[:, 0]).abs().max() <= 1e-12 and (dr.self_sim(edit) - sims[:, 1]).abs().max() <= 1e-12
    assert (dr.score(src, edit) - mse).abs().max() <= 1e-12
    # the all-zero key row: its cosines are 0, not NaN (the clamp is on the product of the norms), and the score stays finite
    got = dr.self_sim(src[8])
    assert torch.isfinite(got).all() and (got[row] == 0).all() and (got[:, row] == 0).all() and (sims[8, 0, row] == 0).all()
    assert torch.isfinite(dr.score(src[8:], edit[8:])).all() and abs(float(mse[8]) - float(mse[0])) > 1e-4


@pytest.mark.parametrize("case", list(dr.CASES))
def test_fixture_keys_and_scores_are_dino_refs(z, case):
    sd, x, b = dr.case_inputs(case)
    k = dr.image_keys(sd, x, -1, 1)
    stride = int(z[f"stride_{case}"])
    assert stride == dr.CASES[case]["stride"]
    assert (k[:, ::stride] - torch.from_numpy(z[f"keys_{case}"])).abs().max() <= 1e-12
    s = dr.score(k[:b], k[b:])
    assert (s - torch.from_numpy(z[f"score_{case}"])).abs().max() <= 1e-12 and s.min() > 1e-3
    for name in ("float16", "bfloat16", "float32"):
        assert 0 < float(z[f"y_K_{case}_{name}"]) < 0.1 and 0 < float(z[f"y_S_{case}_{name}"]) < 0.1
    assert float(z["y_S_a20_float16"]) == float(z["y_S_a64_float16"])          # case A's score yardstick is over the 16 pairs of both sizes


def test_whole_pipeline_is_the_references_class(z):
    """the reference's DinoVitStructure.forward on a seeded 12-block model (see make_dino_golden.py) against dino_ref's resize, tower, keys,
    self-similarity and score"""
    e = dr.E2E
    sd = dr.random_state_dict(**{k: e[k] for k in ("width", "layers", "patch", "image", "seed")})
    src, edit = dr.make_images(1, e["s"], -1, 1, e["image_seed"])
    k = dr.image_keys(sd, torch.cat([src, edit]), -1, 1)
    got, want = float(dr.score(k[:1], k[1:])[0]), float(z["ref_e2e"])
    print(f"dino-ref end to end: {got:.12g} against the reference's {want:.12g}")
    assert k.shape == (2, 785, 384) and abs(got - want) <= 1e-10 * want
