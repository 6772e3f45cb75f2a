"""CPU-only checks of the CLIP metrics' host side: the C ABI's declarations and refusals, the class surface, what EditMetric builds and refuses,
the caption templates, the 77-token limit, and compute_metrics.py on a four-image sweep (plain-torch float32 path, synthetic weights)."""
import ctypes
import inspect
import json
import math
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden"
NEW_SYMBOLS = ["etainv_clip_preprocess", "etainv_clip_assemble_tokens", "etainv_op_vit_attention", "etainv_clip_embed_head", "etainv_clip_similarity"]
OLD_REFUSAL = ("metric 'clip_text_img' is not built: built are ssim, msssim, mse, psnr; the others (clip_text_img, clip_img_img, clip_text_text, "
               "clip_textdir_imgdir, clip_text_img_acc, clip_text_text_acc, dinovitstruct, dinovitstruct_v2, lpips, bglpips, nslpips) need pretrained "
               "CLIP / DINO / LPIPS weights")


def test_new_symbols_are_declared_listed_and_exported():
    from etainv import _capi
    header = (ROOT / "include" / "etainv.h").read_text()
    lib = ctypes.CDLL(str(_capi.lib_path()))
    for name in NEW_SYMBOLS:
        assert name in _capi.SIGNATURES, name
        assert f"int {name}(" in header, name
        assert hasattr(lib, name), name
        decl = header.split(f"int {name}(", 1)[1].split(");", 1)[0]
        assert len(decl.split(",")) == len(_capi.SIGNATURES[name]), name
    for cited in ("clip_similarity.py:223-239", "clip_similarity.py:204-205", ":257-273", ":317-321", ":118-125"):
        assert cited in header, cited
    assert lib.etainv_abi_version() == 1


def test_abi_refusals_by_message():
    from etainv import _capi
    lib = _capi.load()
    p = 0x10000                       # a stand-in pointer: every refusal below is made before anything touches the device
    err = lambda: lib.etainv_last_error().decode()
    pre = lambda **k: lib.etainv_clip_preprocess(*[{**dict(x=p, b=1, s=48, r=32, p=16, lo=-1.0, hi=1.0, bh=p, ch=p, kh=7, bv=p, cv=p, kv=7, rows=24,
                                                         out=p, u8=None, dt=_capi.F16, st=None), **k}[n]
                                                   for n in ("x", "b", "s", "r", "p", "lo", "hi", "bh", "ch", "kh", "bv", "cv", "kv", "rows", "out", "u8", "dt", "st")])
    assert pre(x=None) != 0 and "null pointer" in err() and "etainv_clip_preprocess" in err()
    assert pre(out=None) != 0 and "null pointer" in err()
    assert pre(p=15) != 0 and "patch size must be 14, 16 or 32" in err()
    assert pre(r=40) != 0 and "multiple of the patch size" in err()
    assert pre(s=16384, rows=4096) != 0 and "LDS" in err()
    assert lib.etainv_op_vit_attention(p, p, 1, 5, 2, 40, _capi.F16, None) != 0 and "head_dim 64" in err()
    assert lib.etainv_op_vit_attention(None, p, 1, 5, 2, 64, _capi.F16, None) != 0 and "null pointer" in err()
    assert lib.etainv_op_vit_attention(p + 2, p, 1, 5, 2, 64, _capi.F16, None) != 0 and "16-byte aligned" in err()
    assert lib.etainv_clip_embed_head(None, 0, None, 1, 5, 64, None, None, 1e-5, p, 0, 64, p, None) != 0 and "null pointer" in err()
    assert lib.etainv_clip_embed_head(p, 0, None, 1, 5, 64, None, p, 1e-5, p, 0, 64, p, None) != 0 and "beta without gamma" in err()
    assert lib.etainv_clip_assemble_tokens(p, None, p, p, 1, 4, 64, _capi.F16, None) != 0 and "null pointer" in err()
    assert lib.etainv_clip_similarity(p, p, p, p, 1, 1, 64, 5, p, None) != 0 and "unknown metric mode" in err()
    assert lib.etainv_clip_similarity(p, p, p, p, 1, 1, 64, -1, p, None) != 0 and "unknown metric mode" in err()
    assert lib.etainv_clip_similarity(None, p, p, p, 1, 1, 64, 4, p, None) != 0 and "img_src is required" in err()
    assert lib.etainv_clip_similarity(p, p, p, p, 1, 0, 64, 0, p, None) != 0 and "at least 1" in err()
    assert lib.etainv_clip_similarity(p, p, None, p, 1, 1, 64, 2, p, None) != 0 and "txt_src is required" in err()
    assert lib.etainv_clip_similarity(p, None, p, p, 1, 1, 64, 0, p, None) != 0 and "null pointer" in err()


def test_class_surface_and_reprs():
    from metrics import CLIPAccuracy, CLIPSimilarity, ClipModel, EditMetric, SimpleMetric
    for cls in (CLIPSimilarity, CLIPAccuracy):
        par = inspect.signature(cls.__init__).parameters
        assert list(par) == ["self", "input_range", "device", "use_imagenet_templates", "metric", "clip_model", "weights", "templates"]
        assert [par[k].default for k in list(par)[1:]] == [(-1, 1), None, False, "text_img", "ViT-B/16", None, None]
        assert issubclass(cls, SimpleMetric)
        assert list(inspect.signature(cls.forward).parameters) == ["self", "source_image", "target_image", "source_prompt", "target_prompt"]
    model = ClipModel("synthetic", "cpu", "tiny/16")
    for metric in ("text_img", "img_img", "textdir_imgdir"):
        assert repr(CLIPSimilarity(device="cpu", metric=metric, weights=model)) == f"clip_{metric}"
        assert repr(EditMetric(f"clip_{metric}", device="cpu", clip_weights=model)) == f"clip_{metric}"
    assert repr(CLIPAccuracy(device="cpu", weights=model)) == "clip_text_img_acc"
    assert repr(EditMetric("clip_text_img_acc", device="cpu", clip_weights=model)) == "clip_text_img_acc"
    assert EditMetric.get_built_metrics() == ["ssim", "msssim", "mse", "psnr"] and len(EditMetric.get_available_metrics()) == 14
    with pytest.raises(ValueError, match="weights="):
        CLIPSimilarity(device="cpu")
    with pytest.raises(ValueError, match="square"):
        CLIPSimilarity(device="cpu", weights=model)(target_image=torch.zeros(1, 3, 32, 40), target_prompt="a cat")
    with pytest.raises(ValueError, match="one example per call"):
        CLIPSimilarity(device="cpu", weights=model)(target_image=torch.zeros(2, 3, 32, 32), target_prompt="a cat")


def test_trained_weights_refuse_the_stand_in_tokenizer(tmp_path, monkeypatch):
    """weights that are not synthetic, and no CLIP tokenizer at hand: string prompts are refused (the stand-in's ids lie inside CLIP's vocabulary
    and would score silently wrong); token ids and the image-only metric still work; a tokenizer handed over lifts the refusal"""
    from etainv.weights import synthetic_clip_state_dict
    from metrics import ClipModel, EditMetric, clip_scores
    from metrics.clip_similarity import GEOMETRY
    from modules.utils.tokenizer import WordLevelTokenizer
    monkeypatch.delenv("ETAINV_SD_PATH", raising=False)
    sd = synthetic_clip_state_dict(**GEOMETRY["tiny/16"])              # a state dict handed over: to the model these are trained weights
    model = ClipModel(sd, "cpu")
    assert not model.synthetic and isinstance(model.tokenizer, WordLevelTokenizer)
    x = torch.rand(1, 3, 32, 32) * 2 - 1
    for call in (lambda: model.tokenize(["a cat"]), lambda: model.embed_prompts(["a cat"]),
                 lambda: clip_scores(x, x, ["a cat"], ["a dog"], "clip_text_img", model),
                 lambda: EditMetric("clip_text_img", device="cpu", clip_weights=model).update(x, x, "a cat", "a dog", "dog")):
        with pytest.raises(ValueError, match="ETAINV_SD_PATH") as e:
            call()
        assert "--clip_tokenizer" in str(e.value) and "tokenizer=" in str(e.value) and "stand-in" in str(e.value)
    ids = ClipModel("synthetic", "cpu", "tiny/16").tokenize(["a cat", "a dog"])
    assert clip_scores(x, x, ids[:1], ids[1:], "clip_text_img", model)["clip_text_img"].shape == (1,)        # token ids are taken as they are
    assert clip_scores(x, x, ["a cat"], ["a dog"], "clip_img_img", model)["clip_img_img"].shape == (1,)      # no text pass
    own = ClipModel(sd, "cpu", tokenizer=type("Mine", (), {"encode": lambda self, t: [49406, 7, 49407]})())
    assert own.tokenize(["anything"])[0, :4].tolist() == [49406, 7, 49407, 0]
    with pytest.raises(FileNotFoundError, match="vocab.json"):
        ClipModel(sd, "cpu", tokenizer=str(tmp_path))
    # the command line refuses before it claims a yaml; the image-only metric runs
    import compute_metrics
    assert compute_metrics.parse_args(["--data_path", "a", "--output", "b", "--clip_tokenizer", "dir"]).clip_tokenizer == "dir"
    root, out, stems, _, _ = _sweep(tmp_path)
    weights = tmp_path / "tiny_clip.pt"
    torch.save(sd, weights)
    args = ["--data_path", str(root), "--output", str(out), "--device", "cpu", "--size", "32", "--clip_weights", str(weights)]
    with pytest.raises(ValueError, match="--clip_tokenizer"):
        compute_metrics.main(args + ["--metric", "clip_text_img", "clip_img_img"])
    assert not list((out / "metrics").glob("*.yaml"))
    compute_metrics.main(args + ["--metric", "clip_img_img"])
    assert [f.name for f in (out / "metrics").glob("*.yaml")] == ["clip_img_img.yaml"]


def test_refusals_with_and_without_weights():
    from metrics import CLIPAccuracy, CLIPSimilarity, EditMetric
    with pytest.raises(NotImplementedError) as e:
        EditMetric("clip_text_img")
    assert str(e.value) == OLD_REFUSAL
    for name in ("clip_text_text", "clip_text_text_acc"):
        with pytest.raises(NotImplementedError, match="BLIP"):
            EditMetric(name, clip_weights="synthetic")
        with pytest.raises(NotImplementedError, match="pretrained CLIP / DINO / LPIPS weights"):
            EditMetric(name)
    with pytest.raises(NotImplementedError, match="BLIP"):
        CLIPSimilarity(device="cpu", metric="text_text", weights="synthetic")
    with pytest.raises(NotImplementedError, match="BLIP"):
        CLIPAccuracy(device="cpu", metric="text_text", weights="synthetic")
    with pytest.raises(NotImplementedError, match="pretrained CLIP / DINO / LPIPS weights"):
        EditMetric("lpips", clip_weights="synthetic")


def test_templates_are_the_callers():
    from metrics import CLIPSimilarity, ClipModel, clip_scores
    with pytest.raises(ValueError, match="templates="):
        CLIPSimilarity(device="cpu", use_imagenet_templates=True, weights="synthetic", clip_model="tiny/16")
    with pytest.raises(ValueError, match="templates="):
        ClipModel("synthetic", "cpu", "tiny/16", templates=["no placeholder"])
    plain = ClipModel("synthetic", "cpu", "tiny/16")
    three = ClipModel("synthetic", "cpu", "tiny/16", templates=["a photo of a {}.", "a drawing of the {}.", "{}"])
    assert plain.templates == ["{}"] and plain.captions("cat") == ["cat"]
    assert three.captions("a cat") == ["a photo of a cat.", "a drawing of a cat.", "a cat"]           # 'a a' and 'the a' collapse
    m = CLIPSimilarity(device="cpu", use_imagenet_templates=True, weights="synthetic", clip_model="tiny/16", templates=three.templates)
    assert m.templates == three.templates
    x = torch.rand(1, 3, 32, 32) * 2 - 1
    e3 = three.embed_prompts(["a cat"])
    assert e3.shape == (1, 3, 64) and torch.allclose(e3.norm(dim=-1), torch.ones(1, 3), atol=1e-5)
    mean = e3[0].double().mean(0)
    want = float(three.embed_images(x)[0].double() @ (mean / mean.norm()))
    got = float(clip_scores(x, x, ["a dog"], ["a cat"], "clip_text_img", three)["clip_text_img"][0])
    assert abs(got - want) < 1e-6 and abs(got - float(m(target_image=x, target_prompt="a cat"))) < 1e-6
    assert torch.allclose(e3[0, 2], plain.embed_prompts(["a cat"])[0, 0], atol=1e-6)       # (the CPU path's matmuls depend on the batch)


def test_a_prompt_longer_than_77_tokens_is_refused():
    from metrics import CLIPSimilarity, ClipModel
    from metrics.clip_similarity import PromptTooLong
    model = ClipModel("synthetic", "cpu", "tiny/16")
    assert model.tokenize(["w " * 75]).shape == (1, 77)                                      # 75 words + start + end: the longest that fits
    assert model.tokenize(["a cat"])[0, 3] == 49407 and model.tokenize(["a cat"])[0, 4:].eq(0).all()
    with pytest.raises(RuntimeError, match="too long for context length 77"):
        model.tokenize(["w " * 76])
    m = CLIPSimilarity(device="cpu", weights=model)
    x = torch.zeros(1, 3, 32, 32)
    with pytest.raises(PromptTooLong):
        m(target_image=x, target_prompt="w " * 76)
    assert m.update(target_image=x, target_prompt="w " * 76) is None and m.losses == []      # SimpleMetric: None is not recorded
    assert isinstance(m.update(target_image=x, target_prompt="a cat"), float) and len(m.losses) == 1


def test_edit_metric_routes_by_keyword_and_equals_clip_scores():
    from metrics import ClipModel, EditMetric, clip_scores
    model = ClipModel("synthetic", "cpu", "tiny/16")
    g = torch.Generator().manual_seed(0)
    src, edit = torch.rand(2, 3, 48, 48, generator=g) * 2 - 1, torch.rand(2, 3, 48, 48, generator=g) * 2 - 1
    sp, tp = ["a cat on a bench", "a red car"], ["a dog on a bench", "a blue car"]
    names = ["clip_text_img", "clip_img_img", "clip_textdir_imgdir", "clip_text_img_acc"]
    both = clip_scores(edit, src, sp, tp, names, model)
    for name in names:
        assert both[name].shape == (2,) and both[name].dtype == torch.float32
        m = EditMetric(name, device="cpu", clip_weights=model)
        vals = [m.update(src[i:i + 1], edit[i:i + 1], sp[i], tp[i], "word") for i in range(2)]
        assert all(isinstance(v, float) for v in vals)
        alone = [float(clip_scores(edit[i:i + 1], src[i:i + 1], sp[i:i + 1], tp[i:i + 1], name, model)[name][0]) for i in range(2)]
        assert vals == alone and np.allclose(vals, both[name].numpy(), atol=1e-6)
        mean, info = m.compute()
        assert mean == float(np.mean(vals)) and info["all"] == vals
    assert set(both["clip_text_img_acc"].tolist()) <= {0.0, 1.0}
    same = clip_scores(edit, edit, sp, sp, ["clip_img_img", "clip_text_img_acc", "clip_textdir_imgdir"], model)
    assert np.allclose(same["clip_img_img"].numpy(), 1.0, atol=1e-6) and same["clip_text_img_acc"].tolist() == [0.0, 0.0]
    assert same["clip_textdir_imgdir"].tolist() == [0.0, 0.0]


def _sweep(tmp_path, size=40):
    """a data set of four entries with square images and the imgs/ directory an eval.py sweep leaves, all four pairs complete"""
    from PIL import Image
    from dataset.pie_bench_data import edit_image_name
    entries = list(json.loads((GOLDEN / "pie_bench.json").read_text())["mapping"].items())[:4]
    root, out = tmp_path / "pie", tmp_path / "res"
    (out / "imgs").mkdir(parents=True)
    rng = np.random.default_rng(1)
    stems, prompts = [], []
    strip = lambda s: s.replace("[", "").replace("]", "")
    for i, (key, e) in enumerate(entries):
        f = root / "annotation_images" / e["image_path"]
        f.parent.mkdir(parents=True, exist_ok=True)
        img = rng.integers(0, 256, (size, size, 3), dtype=np.uint8)
        Image.fromarray(img).save(f)
        prompts.append((strip(e["original_prompt"]), strip(e["editing_prompt"])))
        stems.append(edit_image_name(i, *prompts[-1]))
        Image.fromarray((img // 2 + rng.integers(0, 64, img.shape)).astype(np.uint8)).save(out / "imgs" / f"{stems[-1]}.png")
    (root / "mapping_file.json").write_text(json.dumps(dict(entries)))
    return root, out, stems, prompts, [root / "annotation_images" / e["image_path"] for _, e in entries]


def test_compute_metrics_cli_with_clip_weights(tmp_path):
    import yaml
    import compute_metrics
    from metrics import ClipModel, clip_scores
    from modules.models import StablePreprocess
    root, out, stems, prompts, files = _sweep(tmp_path)
    args = ["--data_path", str(root), "--output", str(out), "--device", "cpu", "--size", "32", "--batch", "3", "--limit", "4"]
    with pytest.raises(NotImplementedError, match="pretrained CLIP / DINO / LPIPS weights"):
        compute_metrics.main(args + ["--metric", "clip_text_img"])
    assert not list((out / "metrics").glob("*.yaml")) if (out / "metrics").exists() else True
    tpl = tmp_path / "templates.txt"
    tpl.write_text("a photo of a {}.\n{}\n")
    compute_metrics.main(args + ["--metric", "clip_text_img", "clip_text_img_acc", "mse", "--clip_weights", "synthetic", "--clip_model", "tiny/16",
                                 "--clip_templates", str(tpl)])
    pre = StablePreprocess("cpu", size=32, center_crop=True)
    model = ClipModel("synthetic", "cpu", "tiny/16", templates=["a photo of a {}.", "{}"])
    edits, sources = torch.cat([pre(out / "imgs" / f"{s}.png") for s in stems]), torch.cat([pre(f) for f in files])
    want = clip_scores(edits, sources, [p[0] for p in prompts], [p[1] for p in prompts], ["clip_text_img", "clip_text_img_acc"], model)
    for name in ("clip_text_img", "clip_text_img_acc", "mse"):
        res = yaml.safe_load((out / "metrics" / f"{name}.yaml").read_text())
        assert set(res) == {"name", "mean", "results"} and res["name"] == name
        assert [r["file"] for r in res["results"]] == stems and all(set(r) == {"value", "file"} for r in res["results"])
        vals = [r["value"] for r in res["results"]]
        assert all(isinstance(v, float) and math.isfinite(v) for v in vals) and res["mean"] == float(np.mean(vals))
        if name != "mse":
            assert np.allclose(vals, want[name].numpy(), atol=1e-6), name                    # (batches of 3 + 1 against one batch of 4)
    # a prompt that does not fit gives nan for that sample only
    mapping = json.loads((root / "mapping_file.json").read_text())
    first = next(iter(mapping))
    mapping[first]["editing_prompt"] = "w " * 80
    (root / "mapping_file.json").write_text(json.dumps(mapping))
    from dataset.pie_bench_data import edit_image_name
    long_stem = edit_image_name(0, prompts[0][0], ("w " * 80))
    try:
        (out / "imgs" / f"{long_stem}.png").write_bytes((out / "imgs" / f"{stems[0]}.png").read_bytes())
    except OSError as exc:
        pytest.skip(f"the long-prompt tail needs a file name of {len(long_stem) + 4} characters, which this file system refuses: {exc}")
    (out / "metrics" / "clip_text_img.yaml").unlink()
    compute_metrics.main(args + ["--metric", "clip_text_img", "--clip_weights", "synthetic", "--clip_model", "tiny/16"])
    vals = [r["value"] for r in yaml.safe_load((out / "metrics" / "clip_text_img.yaml").read_text())["results"]]
    assert math.isnan(vals[0]) and all(math.isfinite(v) for v in vals[1:])
