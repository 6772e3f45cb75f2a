"""The CLIP metrics end to end on the device: preprocess, towers, head and scores of a tiny model, against float64.

Fixture model (tests/golden/clip_ref.npz, written by tests/golden/make_clip_golden.py): a randomly initialised transformers CLIPModel; case A at
image size 32 (5 image tokens, two layers), case B its first layer at image size 224 (197 tokens, B = 2).  With e = max |f_gpu - f_64| over the
unit embeddings and y = max |f_prec - f_64| of the same model run by torch on the CPU in that dtype (recorded in the fixture), the test requires
e <= 4 y: y is one draw of a maximum of rounding noise over a few hundred elements (it moves by about 2 x between seeds), and the kernels round at
other points than torch's CPU path.  The library's synthetic weights at the "tiny/16" geometry are held to the same rule: the fixture records
their float64 embeddings and their y as well (the weights themselves are a function of their names).
Scores: |score_gpu - score_64| <= 2 (e_img + e_txt) for the three dot products of unit vectors (img_img: 2 (e_img + e_img)); acc equals the
float64 value, whose margin |sim_tgt - sim_src| exceeds 2 (4 y_img + 4 y_txt) in every pair (asserted on the fixture without a GPU:
tests/test_clip_ref.py).
Measured e / y on MI355X: DESIGN.md, note `clip`."""
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import clip_ref as cr

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / "golden"
DTYPES = [torch.float16, torch.bfloat16, torch.float32]
NAMES = ["clip_text_img", "clip_img_img", "clip_textdir_imgdir", "clip_text_img_acc"]
name_of = lambda dt: str(dt).split(".")[-1]


def load_fixture():
    z = np.load(GOLDEN / "clip_ref.npz")
    sd = {}
    for k in z.files:
        if k.startswith("w:") and k != "w:pos_b":
            e = z["e:" + k[2:]] if "e:" + k[2:] in z.files else None
            sd[k[2:]] = torch.from_numpy(z[k].astype(np.float32)) * (2.0 ** -int(e) if e is not None else 1.0)
    sd["logit_scale"] = torch.tensor(2.6592)
    sd_b = {k: v for k, v in sd.items() if not k.startswith("vision_model.encoder.layers.1.")}
    sd_b["vision_model.embeddings.position_embedding.weight"] = torch.from_numpy(z["w:pos_b"].astype(np.float32)) * 2.0 ** -int(z["e:pos_b"])
    x = lambda u8: torch.from_numpy(u8).float() / 127.5 - 1.0
    return {"z": z, "sd_a": sd, "sd_b": sd_b, "x_a": x(z["img_a_u8"]), "x_b": x(z["img_b_u8"]), "ids": torch.from_numpy(z["ids"].astype(np.int64)),
            "f64": {k: torch.from_numpy(z["f64_" + k]) for k in ("img_a", "img_b", "txt", "syn_img", "syn_txt")}}


@pytest.fixture(scope="module")
def fx():
    return load_fixture()


def _model(sd, dtype):
    from metrics import ClipModel
    return ClipModel(sd, "cuda", compute_dtype=dtype)


def _check(label, got, f64, y):
    e = (got.double().cpu() - f64).abs().max().item()
    print(f"clip-e2e {label}: e {e:.3e} y {y:.3e} e/y {e / y:.2f}")
    assert e <= 4 * y, (label, e, y)
    return e


@pytest.mark.parametrize("dtype", DTYPES, ids=name_of)
def test_fixture_model_embeddings_and_scores(fx, dtype):
    from metrics import clip_scores
    z, f64, nm = fx["z"], fx["f64"], name_of(dtype)
    model = _model(fx["sd_a"], dtype)
    assert (model.patch, model.image, model.backend.proj) == (16, 32, 64)
    img = model.embed_images(fx["x_a"].cuda())
    txt = model.embed_prompts(fx["ids"])
    assert img.dtype == torch.float32 and img.shape == (8, 64) and txt.shape == (8, 1, 64)
    e_img = _check(f"fixture A image 5 tokens {nm}", img, f64["img_a"], float(z[f"y_img_a_{nm}"]))
    e_txt = _check(f"fixture text {nm}", txt[:, 0], f64["txt"], float(z[f"y_txt_{nm}"]))
    got = clip_scores(fx["x_a"][4:].cuda(), fx["x_a"][:4].cuda(), fx["ids"][:4], fx["ids"][4:], NAMES, model)
    want = {n: cr.scores(n[5:], f64["img_a"][:4], f64["img_a"][4:], f64["txt"][:4, None], f64["txt"][4:, None]) for n in NAMES}
    for n in NAMES[:3]:
        d = (got[n].double().cpu() - want[n]).abs().max().item()
        bound = 2 * (2 * e_img if n == "clip_img_img" else e_img + e_txt)
        print(f"clip-e2e score {n} {nm}: delta {d:.3e} bound {bound:.3e}")
        assert d <= bound, (n, d, bound)
    assert torch.equal(got["clip_text_img_acc"].double().cpu(), want["clip_text_img_acc"])


@pytest.mark.parametrize("dtype", DTYPES, ids=name_of)
def test_fixture_model_at_197_tokens(fx, dtype):
    model = _model(fx["sd_b"], dtype)
    assert (model.patch, model.image) == (16, 224) and model.backend.vision.g2 + 1 == 197
    img = model.embed_images(fx["x_b"].cuda())
    _check(f"fixture B image 197 tokens {name_of(dtype)}", img, fx["f64"]["img_b"], float(fx["z"][f"y_img_b_{name_of(dtype)}"]))


@pytest.mark.parametrize("dtype", DTYPES, ids=name_of)
def test_synthetic_weights(fx, dtype):
    from etainv.weights import synthetic_clip_state_dict
    from metrics import ClipModel
    from metrics.clip_similarity import GEOMETRY
    model = ClipModel("synthetic", "cuda", "tiny/16", compute_dtype=dtype)
    x, z, nm = fx["x_a"], fx["z"], name_of(dtype)
    prompts = ["a cat on a bench", "a photo of a red car", "dog", "a blue car in the rain"]         # those of tests/golden/make_clip_golden.py
    if dtype == torch.float32:                                        # once: the recorded float64 values are those of today's synthetic weights
        sd = synthetic_clip_state_dict(**GEOMETRY["tiny/16"])
        rows = cr.patch_rows(cr.preprocess_u8(x, -1, 1, 32), 16)
        assert (cr.image_features(sd, rows, 8) - fx["f64"]["syn_img"]).abs().max() < 1e-12
        assert (cr.text_features(sd, model.tokenize(prompts)) - fx["f64"]["syn_txt"]).abs().max() < 1e-12
    _check(f"synthetic image {nm}", model.embed_images(x.cuda()), fx["f64"]["syn_img"], float(z[f"y_syn_img_{nm}"]))
    _check(f"synthetic text {nm}", model.embed_prompts(prompts)[:, 0], fx["f64"]["syn_txt"], float(z[f"y_syn_txt_{nm}"]))


def test_scores_do_not_depend_on_the_batch_and_repeat(fx):
    from metrics import clip_scores
    model = _model(fx["sd_a"], torch.float16)
    edit, src = fx["x_a"][4:].cuda(), fx["x_a"][:4].cuda()
    run = lambda sl: clip_scores(edit[sl], src[sl], fx["ids"][:4][sl], fx["ids"][4:][sl], NAMES, model)
    full, again = run(slice(0, 4)), run(slice(0, 4))
    for n in NAMES:
        assert torch.equal(full[n].view(torch.int32), again[n].view(torch.int32)), n
        for i in range(4):
            assert torch.equal(run(slice(i, i + 1))[n].view(torch.int32), full[n][i:i + 1].view(torch.int32)), (n, i)


def test_edit_metric_on_the_device_equals_clip_scores(fx):
    from metrics import EditMetric, clip_scores
    sd = fx["sd_a"]
    model = _model(sd, torch.float16)
    prompts = ["a cat on a bench", "a dog on a bench"]
    # a state dict handed over and no CLIP tokenizer at hand: string prompts are refused, token ids are taken as they are
    with pytest.raises(ValueError, match="stand-in"):
        clip_scores(fx["x_a"][4:5].cuda(), fx["x_a"][:1].cuda(), prompts[:1], prompts[1:], "clip_text_img", model)
    syn = EditMetric("clip_textdir_imgdir", device="cuda", clip_weights="synthetic", clip_model="tiny/16")
    assert repr(syn) == "clip_textdir_imgdir" and syn.metric.model.device == "cuda"
    vals = [syn.update(fx["x_a"][i:i + 1], fx["x_a"][4 + i:5 + i], prompts[0], prompts[1], "dog") for i in range(2)]
    want = clip_scores(fx["x_a"][4:6].cuda(), fx["x_a"][:2].cuda(), [prompts[0]] * 2, [prompts[1]] * 2, "clip_textdir_imgdir", syn.metric.model)
    assert vals == [float(v) for v in want["clip_textdir_imgdir"].cpu()]
    mean, info = syn.compute()
    assert mean == float(np.mean(vals)) and info["all"] == vals
    by_sd = EditMetric("clip_img_img", device="cuda", clip_weights=sd)
    v = by_sd.update(fx["x_a"][:1], fx["x_a"][4:5], "", "", "")
    w = clip_scores(fx["x_a"][4:5].cuda(), fx["x_a"][:1].cuda(), fx["ids"][:1], fx["ids"][4:5], "clip_img_img", by_sd.metric.model)
    assert v == float(w["clip_img_img"][0])
