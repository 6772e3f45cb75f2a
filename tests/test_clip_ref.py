"""Pins tests/clip_ref.py on the CPU: the integer restatement of Pillow's bicubic resize against Pillow itself, the float64 towers against
transformers' CLIPModel in float64, the score formulas against hand-computed values, the 16-bit emulation against deliberately broken variants
of itself, and the OpenAI -> transformers renaming of etainv/weights.py against its inverse written out here."""
import numpy as np
import pytest
import torch

from tests import clip_ref as cr

RESIZES = [(512, 224), (96, 224), (64, 32), (48, 32), (37, 32), (32, 32)]


@pytest.mark.parametrize("s,r", RESIZES)
def test_resize_restatement_equals_pillow(s, r):
    Image = pytest.importorskip("PIL.Image")
    for seed, (lo, hi) in enumerate([(-1, 1), (0, 1)]):
        u8 = cr.to_u8(cr.make_images(1, s, lo, hi, seed=seed + s), lo, hi)[0]                    # [3][s][s]
        pil = np.asarray(Image.fromarray(np.ascontiguousarray(u8.transpose(1, 2, 0))).resize((r, r), Image.BICUBIC)).transpose(2, 0, 1)
        mine = cr.pillow_resize_u8(u8, r)
        assert mine.shape == pil.shape and np.array_equal(mine, pil), f"{int((mine != pil).sum())} bytes differ"
        assert len(np.unique(u8)) > 100 and u8.min() == 0 and u8.max() == 255                    # the input uses the range and both clamps


def test_the_librarys_tables_and_cpu_preprocess_equal_the_restatement():
    from metrics.clip_similarity import clip_preprocess, resize_tables
    for s, r in RESIZES:
        for mine, ref in zip(resize_tables(s, r), cr.resize_tables(s, r)):
            assert mine.dtype == np.int32 and np.array_equal(mine, ref)
    x = cr.make_images(2, 48, -1, 1, seed=5)
    rows, u8 = clip_preprocess(x, (-1, 1), 32, 16, torch.float32, return_u8=True)
    ref_u8 = cr.preprocess_u8(x, -1, 1, 32)
    assert np.array_equal(u8.numpy(), ref_u8)
    assert (rows.double() - cr.patch_rows(ref_u8, 16)).abs().max() < 1e-6


def test_truncation_inputs_truncate():
    for lo, hi in ((-1, 1), (0, 1)):
        u8 = cr.to_u8(cr.truncation_images(32, lo, hi), lo, hi)
        assert np.array_equal(u8.reshape(-1), (np.arange(3 * 32 * 32) % 255).astype(np.uint8))


def test_patch_row_inputs_keep_the_excepted_elements_under_one_percent():
    from tests.test_clip_kernels_gpu import _ref_u8, _rows_check
    for s, r, p in [(48, 32, 16), (48, 32, 32), (37, 28, 14), (32, 32, 16)]:
        f64 = cr.patch_rows(_ref_u8(3, s, r, -1, 1), p)[:, :3 * p * p]
        for dtype in (torch.float16, torch.bfloat16):
            bad, excepted = _rows_check(f64.to(dtype), f64, dtype)
            assert bad == 0 and excepted <= 0.01 * f64.numel(), (s, r, p, dtype, excepted)
        assert _rows_check(f64.float(), f64, torch.float32) == (0, 0)


def tiny_clip(image):
    transformers = pytest.importorskip("transformers")
    torch.manual_seed(image)
    enc = dict(hidden_size=128, num_attention_heads=2, num_hidden_layers=2, intermediate_size=512, projection_dim=64, hidden_act="quick_gelu")
    cfg = transformers.CLIPConfig(text_config=dict(enc, vocab_size=49408, eos_token_id=49407, bos_token_id=49406, max_position_embeddings=77),
                                  vision_config=dict(enc, patch_size=16, image_size=image), projection_dim=64)
    return transformers.CLIPModel(cfg).double().eval()


def tiny_ids(b, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.zeros(b, 77, dtype=torch.int64)
    for i in range(b):
        n = 3 + 5 * i
        ids[i, 0], ids[i, 1:1 + n], ids[i, 1 + n] = 49406, torch.randint(1000, 41000, (n,), generator=g), 49407
    return ids


def _pooled(o):
    return getattr(o, "pooler_output", o)


@pytest.mark.parametrize("image", [32, 64])
def test_float64_towers_equal_transformers(image):
    model = tiny_clip(image)
    sd = {k: v.detach() for k, v in model.state_dict().items()}
    u8 = cr.preprocess_u8(cr.make_images(2, 48, -1, 1, seed=image), -1, 1, image)
    pixels = (torch.from_numpy(u8.astype(np.float64)) / 255.0 - torch.tensor(cr.MEAN, dtype=torch.float64).view(1, 3, 1, 1)) \
        / torch.tensor(cr.STD, dtype=torch.float64).view(1, 3, 1, 1)
    ids = tiny_ids(3, seed=image)
    with torch.no_grad():
        want_img = _pooled(model.get_image_features(pixel_values=pixels))
        want_txt = _pooled(model.get_text_features(input_ids=ids))
    rel = lambda a, b: ((a - b).abs().max() / b.abs().max()).item()
    assert cr.geometry(sd) == {"width": 128, "patch": 16, "image": image, "proj": 64, "text_width": 128}
    assert rel(cr.image_features(sd, cr.patch_rows(u8, 16), 2, normalize=False), want_img) <= 1e-10
    assert rel(cr.text_features(sd, ids, normalize=False), want_txt) <= 1e-10
    unit = cr.image_features(sd, cr.patch_rows(u8, 16), 2)
    assert rel(unit, want_img / want_img.norm(dim=-1, keepdim=True)) <= 1e-10


def test_score_formulas_by_hand():
    t = lambda *rows: torch.tensor(rows, dtype=torch.float64)
    img_tgt, img_src = t([1.0, 0.0], [0.0, 1.0]), t([0.0, 1.0], [0.6, 0.8])
    txt_tgt, txt_src = t([[0.6, 0.8]], [[0.0, 1.0]]), t([[1.0, 0.0]], [[0.8, 0.6]])
    close = lambda a, b: torch.allclose(a, t(*b).reshape(-1), atol=1e-15)
    assert close(cr.scores("text_img", img_tgt=img_tgt, txt_tgt=txt_tgt), [0.6, 1.0])
    assert close(cr.scores("img_img", img_src=img_src, img_tgt=img_tgt), [0.0, 0.8])
    # pair 0: (1, -1) . (-0.4, 0.8) = -1.2 (negative); pair 1: (-0.6, 0.2) . (-0.8, 0.4) = 0.56
    assert close(cr.scores("textdir_imgdir", img_src, img_tgt, txt_src, txt_tgt), [-1.2, 0.56])
    # pair 0: 0.6 against 1.0 for the source prompt -> 0; pair 1: 1.0 against 0.6 -> 1
    assert close(cr.scores("text_img_acc", img_src, img_tgt, txt_src, txt_tgt), [0.0, 1.0])
    # two templates: the mean of (1, 0) and (0, 1) renormalised is (1, 1) / sqrt 2
    two = t([1.0, 0.0], [0.0, 1.0])[None]
    assert close(cr.prompt_embedding(two)[0], [0.5 ** 0.5, 0.5 ** 0.5])
    assert close(cr.scores("text_img", img_tgt=t([1.0, 0.0]), txt_tgt=two), [0.5 ** 0.5])
    assert close(cr.scores("text_img_acc", img_tgt=t([1.0, 0.0]), txt_src=two, txt_tgt=two), [0.0])       # an exact tie is 0


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_emulation_is_worse_than_float64_and_every_rounding_point_counts(dtype):
    sd = cr.random_state_dict(seed=3)
    rows = cr.patch_rows(cr.preprocess_u8(cr.make_images(2, 48, -1, 1, seed=9), -1, 1, 32), 16)
    ids = torch.tensor([[62, 5, 9, 63] + [0] * 73, [62, 7, 63] + [0] * 74])
    for feats, arg in ((lambda pr: cr.image_features(sd, rows, 2, pr), "image"), (lambda pr: cr.text_features(sd, ids, pr), "text")):
        exact, full = feats(cr.Prec()), feats(cr.Prec(dtype))
        assert torch.equal(exact, feats(cr.Prec(None, skip=("p",))))
        err = (full - exact).abs().max().item()
        assert err > 10 * torch.finfo(torch.float32).eps and err < 0.1, (arg, err)
        for point in cr.Prec.POINTS:
            broken = feats(cr.Prec(dtype, skip=(point,)))
            assert not torch.equal(broken, full), f"{arg}: leaving out the rounding at '{point}' changes nothing"


def to_openai(sd):
    """the inverse of etainv.weights.openai_clip_to_transformers, written out"""
    top = {"vision_model.embeddings.patch_embedding.weight": "visual.conv1.weight", "vision_model.embeddings.class_embedding": "visual.class_embedding",
           "vision_model.embeddings.position_embedding.weight": "visual.positional_embedding",
           "vision_model.pre_layrnorm.weight": "visual.ln_pre.weight", "vision_model.pre_layrnorm.bias": "visual.ln_pre.bias",
           "vision_model.post_layernorm.weight": "visual.ln_post.weight", "vision_model.post_layernorm.bias": "visual.ln_post.bias",
           "text_model.embeddings.token_embedding.weight": "token_embedding.weight",
           "text_model.embeddings.position_embedding.weight": "positional_embedding",
           "text_model.final_layer_norm.weight": "ln_final.weight", "text_model.final_layer_norm.bias": "ln_final.bias", "logit_scale": "logit_scale"}
    block = {"layer_norm1": "ln_1", "layer_norm2": "ln_2", "self_attn.out_proj": "attn.out_proj", "mlp.fc1": "mlp.c_fc", "mlp.fc2": "mlp.c_proj"}
    out = {}
    for k, v in sd.items():
        if k in top:
            out[top[k]] = v
        elif k == "visual_projection.weight":
            out["visual.proj"] = v.t().contiguous()
        elif k == "text_projection.weight":
            out["text_projection"] = v.t().contiguous()
        elif ".self_attn.q_proj." in k:
            tower, rest = k.split("encoder.layers.")
            n, kind = rest.split(".")[0], k.rsplit(".", 1)[1]
            base = ("visual.transformer" if tower == "vision_model." else "transformer") + f".resblocks.{n}.attn.in_proj_{kind}"
            out[base] = torch.cat([sd[k.replace("q_proj", p)] for p in ("q_proj", "k_proj", "v_proj")])
        elif ".self_attn.k_proj." in k or ".self_attn.v_proj." in k:
            continue
        else:
            tower, rest = k.split("encoder.layers.")
            n, mod = rest.split(".", 1)
            mod, kind = mod.rsplit(".", 1)
            out[("visual.transformer" if tower == "vision_model." else "transformer") + f".resblocks.{n}.{block[mod]}.{kind}"] = v
    return out


def test_openai_names_convert_back_exactly():
    from etainv.nets import clip_geometry
    from etainv.weights import load_clip_state_dict, openai_clip_to_transformers
    sd = cr.random_state_dict(seed=1)
    oa = to_openai(sd)
    assert "visual.transformer.resblocks.1.attn.in_proj_weight" in oa and oa["visual.proj"].shape == (128, 64) and len(oa) < len(sd)
    back = openai_clip_to_transformers(oa)
    assert set(back) == set(sd)
    for k in sd:
        assert torch.equal(back[k], sd[k]), k
    loaded = load_clip_state_dict(oa)                                  # a plain OpenAI dict is recognised and renamed
    assert set(loaded) == set(sd) and all(torch.equal(loaded[k], sd[k]) for k in sd)
    assert clip_geometry(loaded) == {"width": 128, "layers": 2, "patch": 16, "image": 32, "proj": 64, "text_width": 128, "text_layers": 2, "vocab": 64}


def test_fixture_is_what_the_reference_computes_and_its_margins_hold():
    """tests/golden/clip_ref.npz against tests/clip_ref.py, and the premise of the acc check of tests/test_clip_gpu.py: every pair's float64
    margin |sim_tgt - sim_src| exceeds 2 (4 y_img + 4 y_txt) in every dtype"""
    from tests.test_clip_gpu import DTYPES, load_fixture, name_of
    fx = load_fixture()
    z, f64 = fx["z"], fx["f64"]
    rows = cr.patch_rows(cr.preprocess_u8(fx["x_a"], -1, 1, 32), 16)
    assert (cr.image_features(fx["sd_a"], rows, 8) - f64["img_a"]).abs().max() < 1e-12
    assert (cr.text_features(fx["sd_a"], fx["ids"]) - f64["txt"]).abs().max() < 1e-12
    margin = ((f64["txt"][4:] - f64["txt"][:4]) * f64["img_a"][4:]).sum(-1).abs()
    for dt in DTYPES:
        assert margin.min() > 2 * 4 * (float(z[f"y_img_a_{name_of(dt)}"]) + float(z[f"y_txt_{name_of(dt)}"])), (dt, margin)
    acc = cr.scores("text_img_acc", f64["img_a"][:4], f64["img_a"][4:], f64["txt"][:4, None], f64["txt"][4:, None])
    assert acc.tolist() == [1.0, 0.0, 1.0, 0.0]
