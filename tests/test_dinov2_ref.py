"""Pins tests/dinov2_ref.py without a GPU: the bicubic restatement against F.interpolate in both forms (scale_factor (g + 0.1) / M, the
published hub code's; size (g, g), transformers'), the float64 tower with LayerScale against transformers' Dinov2Model, the fixture's float64 keys
and scores against dinov2_ref as it stands, and the values the reference's own DinoVitStructure and VitExtractor gave on a DINOv2-shaped
stand-in model (recorded in tests/golden/dinov2_ref.npz by tests/golden/make_dinov2_golden.py)."""
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import dinov2_ref as v2

GOLDEN = Path(__file__).resolve().parent / "golden"
U = 2.0 ** -24
MG = [(37, 16), (5, 3), (3, 4), (4, 2)]


@pytest.fixture(scope="module")
def z():
    return np.load(GOLDEN / "dinov2_ref.npz")


def _torch_table(pos, m, g, offset, dtype):
    grid = pos[0, 1:].to(dtype).reshape(1, m, m, -1).permute(0, 3, 1, 2)
    kw = dict(scale_factor=((g + offset) / m, (g + offset) / m)) if offset else dict(size=(g, g))
    out = F.interpolate(grid, mode="bicubic", antialias=False, **kw)
    assert tuple(out.shape[-2:]) == (g, g)
    return torch.cat([pos[0, :1], out.permute(0, 2, 3, 1).reshape(g * g, -1).to(pos.dtype)])          # the class row unchanged


@pytest.mark.parametrize("offset", [0.1, 0.0])
@pytest.mark.parametrize("m,g", MG)
def test_bicubic_restatement_is_torchs(m, g, offset):
    """float64 against float64: 1e-12.  torch's float32 kernel against the float64 restatement: the source coordinate (i + 0.5) scale - 0.5 is
    three fp32 operations on values up to M, so t is off by at most 3 u M; a cubic weight's slope is below 1.5, four taps per axis, two axes,
    plus 40 roundings in the weights and the 16-term sum: (2 * 4 * 1.5 * 3 M + 40) u max|v|"""
    pos = torch.randn(1, 1 + m * m, 8, dtype=torch.float64, generator=torch.Generator().manual_seed(m))
    got = v2.position_table(pos, g, offset)
    want = _torch_table(pos, m, g, offset, torch.float64)
    err32 = (_torch_table(pos, m, g, offset, torch.float32) - got).abs().max().item()
    bound32 = (36 * m + 40) * U * pos.abs().max().item()
    print(f"dinov2-ref bicubic {m}->{g} offset {offset}: float64 max |diff| {(got - want).abs().max():.3e}; float32 {err32:.3e} (bound {bound32:.3e})")
    assert got.shape == want.shape == (1 + g * g, 8) and torch.equal(got[0], pos[0, 0])
    assert (got - want).abs().max() <= 1e-12
    assert err32 <= bound32
    w = v2.bicubic_weights(m, g, m / g)
    assert (w.sum(1) - 1).abs().max() <= 1e-14                      # the cubic convolution weights sum to one


def test_the_two_forms_of_the_table_differ():
    """scale_factor (g + 0.1) / M against size (g, g) on one random model's 37 -> 16 table: not a detail, so using the wrong one cannot pass"""
    sd = v2.random_state_dict(128, 2, 37, seed=22)
    a, b = v2.position_table(sd["pos_embed"], 16, 0.1), v2.position_table(sd["pos_embed"], 16, 0.0)
    diff = (a - b).abs().max().item()
    print(f"dinov2-ref table 37->16: offset 0.1 against offset 0 max |diff| {diff:.3f}")
    assert diff > 0.1
    assert torch.equal(v2.position_table(sd["pos_embed"], 37, 0.1), sd["pos_embed"][0].double())          # g == M: used as it is


# transformers' Dinov2Model names -> the published checkpoints'
def _to_hub_names(sd, layers):
    out = {"cls_token": sd["embeddings.cls_token"], "pos_embed": sd["embeddings.position_embeddings"], "mask_token": sd["embeddings.mask_token"],
           "patch_embed.proj.weight": sd["embeddings.patch_embeddings.projection.weight"],
           "patch_embed.proj.bias": sd["embeddings.patch_embeddings.projection.bias"]}
    for i in range(layers):
        s, p = f"encoder.layer.{i}.", f"blocks.{i}."
        for kind in ("weight", "bias"):
            out[p + f"attn.qkv.{kind}"] = torch.cat([sd[s + f"attention.attention.{n}.{kind}"] for n in ("query", "key", "value")])
            out[p + f"attn.proj.{kind}"] = sd[s + f"attention.output.dense.{kind}"]
            for nm in ("norm1", "norm2", "mlp.fc1", "mlp.fc2"):
                out[p + f"{nm}.{kind}"] = sd[s + f"{nm}.{kind}"]
        out[p + "ls1.gamma"], out[p + "ls2.gamma"] = sd[s + "layer_scale1.lambda1"], sd[s + "layer_scale2.lambda1"]
    return out


def test_keys_are_those_of_transformers_dinov2():
    """image 224 against a 37 x 37 table, so the model's own interpolation (size (16, 16): offset 0) runs.  transformers interpolates in float32
    even in a float64 model: once with dinov2_ref's float64 table (the difference is the float32 kernel's error, bounded as above, through a
    tower of gain O(1): 1e-4), once with torch's float32 table handed to dinov2_ref's tower (1e-10: everything else)"""
    import transformers
    torch.manual_seed(4)
    cfg = transformers.Dinov2Config(hidden_size=128, num_hidden_layers=3, num_attention_heads=2, mlp_ratio=4, image_size=518, patch_size=14,
                                    layer_norm_eps=1e-6, hidden_act="gelu", layerscale_value=1.0)
    model = transformers.Dinov2Model(cfg).double().eval()
    with torch.no_grad():
        for name, p in model.named_parameters():
            if "lambda1" in name:
                p.copy_(torch.pow(10.0, -3.0 * torch.rand(p.shape, dtype=p.dtype)) * (torch.randint(0, 2, p.shape) * 2 - 1))
            elif p.dim() == 1 or "cls_token" in name or "position" in name:
                p.add_(0.1 * torch.randn(p.shape, dtype=p.dtype))
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    names = _to_hub_names(sd, 3)
    assert names["pos_embed"].shape == (1, 1 + 37 * 37, 128) and v2.geometry(names) == {"width": 128, "patch": 14, "image": 224, "table": 37, "layers": 3}
    src, edit = v2.make_images(1, 48, -1, 1, seed=5)
    pix = v2.preprocess(torch.cat([src, edit]), -1, 1, 224)
    taken = []
    hook = model.encoder.layer[-1].attention.attention.key.register_forward_hook(lambda mod, inp, out: taken.append(out.detach()))
    with torch.no_grad():
        model(pixel_values=pix)
    hook.remove()
    rows = v2.patch_rows(pix, 14)
    got = v2.keys(names, rows, 2, offset=0.0)
    same_table = v2.keys(names, rows, 2, offset=0.0, table=_torch_table(names["pos_embed"], 37, 16, 0.0, torch.float32))
    err, err_same = (got - taken[0]).abs().max().item(), (same_table - taken[0]).abs().max().item()
    print(f"dinov2-ref keys against transformers Dinov2Model: max |diff| {err:.3e}, with torch's float32 table {err_same:.3e} (|K| max {taken[0].abs().max():.2f})")
    assert got.shape == taken[0].shape == (2, 257, 128) and err_same <= 1e-10 and err <= 1e-4
    assert (v2.keys(names, rows, 2, offset=0.1) - taken[0]).abs().max() > 1e-3            # the other form is another model


@pytest.mark.parametrize("case", list(v2.CASES))
def test_fixture_keys_and_scores_are_dinov2_refs(z, case):
    sd, image, x, b = v2.case_inputs(case)
    k = v2.image_keys(sd, x, -1, 1, image=image)
    stride = int(z[f"stride_{case}"])
    assert stride == v2.CASES[case]["stride"] and k.shape[1] == {"b": 257}.get(case, 10)
    assert (k[:, ::stride] - torch.from_numpy(z[f"keys_{case}"])).abs().max() <= 1e-12
    s = v2.score(k[:b], k[b:])
    assert (s - torch.from_numpy(z[f"score_{case}"])).abs().max() <= 1e-12 and s.min() > 1e-3
    for name in ("float16", "bfloat16", "float32"):
        assert 0 < float(z[f"y_K_{case}_{name}"]) < 0.1 and 0 < float(z[f"y_S_{case}_{name}"]) < 0.1
    assert float(z["y_S_a20_float16"]) == float(z["y_S_a64_float16"])          # case A's score yardstick is over the 16 pairs of both sizes


def test_random_state_dict_gammas_are_powers_of_two():
    sd, _ = v2.case_model("a")
    g = torch.stack([sd[f"blocks.{i}.{nm}.gamma"] for i in range(3) for nm in ("ls1", "ls2")]).double().abs()
    assert torch.equal(torch.log2(g), torch.log2(g).round()) and g.min() >= 2.0 ** -17 and g.max() <= 1.0 and g.min() < 2.0 ** -12
    for dt in (torch.float16, torch.bfloat16):
        w = sd["blocks.0.attn.proj.weight"]
        assert torch.equal(w.to(dt).float(), w)


def test_whole_pipeline_is_the_references_class(z):
    """the reference's DinoVitStructure.forward(vit_model="dinov2_vits14") and its VitExtractor's keys on a seeded 12-block DINOv2-shaped model
    that interpolates with F.interpolate itself (make_dinov2_golden.py), against dinov2_ref's resize, table, tower, keys and score"""
    e = v2.E2E
    sd = v2.random_state_dict(e["width"], e["layers"], e["table"], e["seed"])
    src, edit = v2.make_images(1, e["s"], -1, 1, e["image_seed"])
    k = v2.image_keys(sd, torch.cat([src, edit]), -1, 1)
    got, want = float(v2.score(k[:1], k[1:])[0]), float(z["ref_e2e"])
    print(f"dinov2-ref end to end: {got:.12g} against the reference's {want:.12g}")
    assert k.shape == (2, 257, 384) and abs(got - want) <= 1e-10 * want
    assert (k[0, ::16] - torch.from_numpy(z["ref_keys"])).abs().max() <= 1e-9
