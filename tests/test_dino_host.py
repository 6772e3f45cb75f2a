"""CPU-only checks of the dinovitstruct metric's host side: the C ABI's declarations and refusals, the table builder, the weight loader, what the
model and EditMetric build and refuse, the CPU float32 path against float64, and compute_metrics.py on a four-image sweep."""
import ctypes
import inspect
import math

import numpy as np
import pytest
import torch

from tests import dino_ref as dr
from tests.test_clip_host import ROOT, _sweep

NEW_SYMBOLS = ["etainv_dino_preprocess", "etainv_op_gelu_erf", "etainv_dino_selfsim_mse"]
OLD_REFUSAL = ("metric 'dinovitstruct' is not built: built are ssim, msssim, mse, psnr; the others (clip_text_img, clip_img_img, clip_text_text, "
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
    assert "int64_t etainv_dino_selfsim_workspace_bytes(int b, int n);" in header and hasattr(lib, "etainv_dino_selfsim_workspace_bytes")
    for cited in ("dino_vit_structure.py:236-241", ":15-20", ":262"):
        assert cited in header, cited


def test_abi_refusals_by_message():
    from etainv import _capi
    lib = _capi.load()
    p = 0x10000                       # a stand-in pointer: every refusal below is made before anything touches the device
    err = lambda: lib.etainv_last_error().decode()
    order = ("x", "b", "s", "r", "p", "lo", "hi", "bh", "ch", "kh", "bv", "cv", "kv", "rows", "out", "dt", "st")
    pre = lambda **k: lib.etainv_dino_preprocess(*[{**dict(x=p, b=1, s=512, r=224, p=8, lo=-1.0, hi=1.0, bh=p, ch=p, kh=5, bv=p, cv=p, kv=5, rows=21,
                                                         out=p, dt=_capi.F16, st=None), **k}[n] for n in order])
    assert pre(x=None) != 0 and "null pointer" in err() and "etainv_dino_preprocess" in err()
    assert pre(out=None) != 0 and "null pointer" in err()
    assert pre(ch=None) != 0 and "null pointer" in err()
    assert pre(out=p + 2) != 0 and "aligned" in err()
    assert pre(x=p + 1) != 0 and "aligned" in err()
    assert pre(p=14) != 0 and "patch size must be 8 or 16" in err()
    assert pre(r=220) != 0 and "multiple of the patch size" in err()
    assert pre(b=65536) != 0 and "65535" in err()
    assert pre(lo=1.0) != 0 and "hi > lo" in err()
    assert pre(s=4096, rows=400) != 0 and "LDS" in err()
    assert pre(b=0) == 0                                              # 512 -> 224 at p = 8 (21 rows of 224 floats) fits; nothing is launched for b = 0
    assert pre(b=0, p=16, rows=40) == 0
    ws = lib.etainv_dino_selfsim_workspace_bytes
    assert ws(1, 785) == 8 * 91 + 2 * 785 * 4 and ws(3, 17) == 3 * 8 + 6 * 17 * 4 and ws(0, 5) == 0
    assert ws(1, 0) == -1 and "n in [1, 16384]" in err()
    order = ("keys", "b", "n", "d", "ld", "eps", "out", "norms", "ws", "bytes", "dt", "st")
    sim = lambda **k: lib.etainv_dino_selfsim_mse(*[{**dict(keys=p, b=1, n=17, d=128, ld=128, eps=1e-8, out=p, norms=None, ws=p, bytes=1 << 20,
                                                         dt=_capi.F16, st=None), **k}[n] for n in order])
    assert sim(keys=None) != 0 and "null pointer" in err() and "etainv_dino_selfsim_mse" in err()
    assert sim(out=None) != 0 and "null pointer" in err()
    assert sim(ws=None) != 0 and "null pointer" in err()
    assert sim(keys=p + 2) != 0 and "16-byte aligned" in err()
    assert sim(ws=p + 4) != 0 and "8-byte aligned" in err()
    assert sim(d=100, ld=104) != 0 and "multiple of 64" in err()
    assert sim(d=0) != 0 and "multiple of 64" in err()
    assert sim(ld=64) != 0 and "row stride" in err()
    assert sim(ld=130) != 0 and "row stride" in err()
    assert sim(eps=0.0) != 0 and "eps must be positive" in err()
    assert sim(eps=float("nan")) != 0 and "eps must be positive" in err()
    assert sim(b=32768) != 0 and "32767" in err()
    assert sim(n=16385) != 0 and "16384" in err()
    assert sim(bytes=16) != 0 and "workspace too small" in err()
    assert sim(dt=7) != 0 and "bad dtype" in err()
    assert sim(b=0) == 0
    assert lib.etainv_op_gelu_erf(None, p, 4, _capi.F16, None) != 0 and "null pointer" in err()
    assert lib.etainv_op_gelu_erf(p, p, -1, _capi.F16, None) != 0 and "n must be" in err()
    assert lib.etainv_op_gelu_erf(p, p, 0, _capi.F16, None) == 0


@pytest.mark.parametrize("antialias", [True, False])
@pytest.mark.parametrize("s,r", [(20, 32), (64, 224), (224, 224), (300, 224), (512, 224)])
def test_table_builder_is_dino_refs(s, r, antialias):
    from metrics.dino_vit_structure import _band_rows, resize_tables
    bounds, coef = resize_tables(s, r, antialias)
    want_b, want_c = dr.resize_tables(s, r, antialias)
    assert bounds.dtype == np.int32 and coef.dtype == np.float64
    assert np.array_equal(bounds, want_b) and np.array_equal(coef, want_c)
    assert not bounds.flags.writeable and not coef.flags.writeable
    for p in (8, 16):
        rows = _band_rows(bounds, p)
        assert rows * r * 4 <= 65536 and rows <= s
        assert rows <= math.ceil((p - 1) * s / r + 2 * max(s / r, 1.0)) + 1          # p - 1 centre steps plus the support on either side


def test_weight_loader_unwraps_strips_and_refuses(tmp_path):
    from etainv.nets import dino_geometry
    from etainv.weights import load_dino_state_dict, synthetic_dino_state_dict
    sd = synthetic_dino_state_dict(width=128, layers=2, patch=8, image=32, seed=1)
    assert sd["pos_embed"].shape == (1, 17, 128) and sd["patch_embed.proj.bias"].shape == (128,) and sd["blocks.1.attn.qkv.weight"].shape == (384, 128)
    again = synthetic_dino_state_dict(width=128, layers=2, patch=8, image=32, seed=1)
    assert all(torch.equal(sd[k], again[k]) for k in sd)
    assert dino_geometry(sd) == {"width": 128, "patch": 8, "layers": 2, "image": 32, "g2": 16}
    wrapped = {"teacher": {"module.backbone." + k: v.half() for k, v in sd.items()}, "student": {}, "epoch": 3}
    wrapped["teacher"]["module.head.last_layer.weight"] = torch.zeros(4, 4)
    for form in (wrapped, {"state_dict": {"backbone." + k: v for k, v in sd.items()}}, sd):
        f = tmp_path / "w.pth"
        torch.save(form, f)
        got = load_dino_state_dict(f)
        assert set(got) == set(sd) and all(v.dtype == torch.float32 for v in got.values())
        assert torch.equal(got["cls_token"], sd["cls_token"].half().float() if form is wrapped else sd["cls_token"])
    assert set(load_dino_state_dict(sd)) == set(sd)
    for extra in ("blocks.0.ls1.gamma", "blocks.0.gamma_1", "register_tokens"):
        with pytest.raises(ValueError, match="DINOv2"):
            load_dino_state_dict({**sd, extra: torch.ones(128)})
        with pytest.raises(ValueError, match="DINOv2"):
            dino_geometry({**sd, extra: torch.ones(128)})
    with pytest.raises(ValueError, match="not a DINO ViT state dict"):
        load_dino_state_dict({"visual.conv1.weight": torch.zeros(1)})
    with pytest.raises(ValueError, match="pos_embed has 18 rows"):
        dino_geometry({**sd, "pos_embed": torch.zeros(1, 18, 128)})
    with pytest.raises(ValueError, match="multiple of 64"):
        dino_geometry({**sd, "patch_embed.proj.weight": torch.zeros(96, 3, 8, 8)})
    with pytest.raises(ValueError, match="8 x 8 or 16 x 16"):
        dino_geometry({**sd, "patch_embed.proj.weight": torch.zeros(128, 3, 14, 14)})
    big = {**sd, "pos_embed": torch.zeros(1, 785, 128)}
    assert dino_geometry(big)["image"] == 224 and dino_geometry({**sd, "patch_embed.proj.weight": torch.zeros(128, 3, 16, 16),
                                                                 "pos_embed": torch.zeros(1, 197, 128)})["image"] == 224


def test_class_surface_reprs_and_refusals():
    from metrics import DinoModel, DinoVitStructure, EditMetric, SimpleMetric, dino_structure
    from metrics.dino_vit_structure import GEOMETRY
    assert set(GEOMETRY) == {"dino_vitb8", "dino_vits8", "dino_vitb16", "dino_vits16", "tiny/8"}
    assert GEOMETRY["dino_vitb8"] == dict(width=768, layers=12, patch=8, image=224)
    par = inspect.signature(DinoVitStructure.__init__).parameters
    assert list(par)[:4] == ["self", "input_range", "device", "vit_model"] and par["vit_model"].default == "dino_vitb8"
    assert list(inspect.signature(DinoVitStructure.forward).parameters) == ["self", "pred", "target"] and issubclass(DinoVitStructure, SimpleMetric)
    par = inspect.signature(DinoModel.__init__).parameters
    assert list(par)[:6] == ["self", "weights", "device", "dino_model", "compute_dtype", "antialias"]
    assert (par["dino_model"].default, par["compute_dtype"].default, par["antialias"].default) == ("dino_vitb8", torch.float16, True)
    model = DinoModel("synthetic", "cpu", "tiny/8")
    assert (model.patch, model.image, model.width, model.antialias) == (8, 32, 128, True)
    assert DinoModel(model, "cpu").backend is model.backend                                                   # a loaded model is shared
    assert repr(DinoVitStructure(device="cpu", vit_model="tiny/8", weights=model)) == "tiny/8"
    assert repr(EditMetric("dinovitstruct", device="cpu", dino_weights=model, dino_model="dino_vitb8")) == "dino_vitb8"
    assert EditMetric.get_built_metrics() == ["ssim", "msssim", "mse", "psnr"] and len(EditMetric.get_available_metrics()) == 14
    with pytest.raises(ValueError, match="weights="):
        DinoVitStructure(device="cpu")
    with pytest.raises(ValueError, match="square"):
        model.keys(torch.zeros(1, 3, 32, 40))
    with pytest.raises(ValueError, match="square"):
        dino_structure(torch.zeros(1, 3, 32, 40), torch.zeros(1, 3, 32, 40), model)
    with pytest.raises(ValueError, match="same dimensions"):
        dino_structure(torch.zeros(1, 3, 32, 32), torch.zeros(1, 3, 40, 40), model)
    with pytest.raises(ValueError, match="dino_model must be one of"):
        DinoModel("synthetic", "cpu", "dino_vitl8")
    with pytest.raises(NotImplementedError, match="LayerScale"):
        DinoModel("synthetic", "cpu", "dinov2_vitb14")
    with pytest.raises(NotImplementedError) as e:
        EditMetric("dinovitstruct")
    assert str(e.value) == OLD_REFUSAL
    with pytest.raises(NotImplementedError, match="pretrained CLIP / DINO / LPIPS weights"):
        EditMetric("dinovitstruct", clip_weights="synthetic")
    with pytest.raises(NotImplementedError, match="pretrained CLIP / DINO / LPIPS weights"):
        EditMetric("dinovitstruct_v2")
    with pytest.raises(NotImplementedError) as e:
        EditMetric("dinovitstruct_v2", dino_weights="synthetic")
    assert all(w in str(e.value) for w in ("patch 14", "LayerScale", "interpolated position embeddings"))
    with pytest.raises(NotImplementedError, match="pretrained CLIP / DINO / LPIPS weights"):
        EditMetric("lpips", dino_weights="synthetic")


def test_edit_metric_passes_source_then_edit_and_equals_dino_structure():
    from metrics import DinoModel, EditMetric, dino_structure
    model = DinoModel("synthetic", "cpu", "tiny/8")
    src, edit = dr.make_images(2, 40, -1, 1, seed=9)
    both = dino_structure(edit, src, model)
    assert both.shape == (2,) and both.dtype == torch.float64 and (both > 0).all()
    m = EditMetric("dinovitstruct", device="cpu", dino_weights=model, dino_model="tiny/8")
    seen = []
    inner = m.metric.forward
    m.metric.forward = lambda pred, target: (seen.append((pred, target)), inner(pred, target))[1]
    vals = [m.update(src[i:i + 1], edit[i:i + 1], "a cat", "a dog", "dog") for i in range(2)]
    assert all(isinstance(v, float) for v in vals)
    assert seen[0][0] is not None and torch.equal(seen[0][0], src[:1]) and torch.equal(seen[0][1], edit[:1])     # (source_image, edit_image)
    alone = [float(dino_structure(src[i:i + 1], edit[i:i + 1], model)[0]) for i in range(2)]
    assert vals == alone and np.allclose(vals, both.numpy(), rtol=1e-5)
    mean, info = m.compute()
    assert mean == float(np.mean(vals)) and info["all"] == vals
    assert float(dino_structure(edit, edit, model).abs().max()) == 0.0
    # a batch handed to the class gives the sum over its pairs, as the reference's loop does
    assert abs(float(m.metric(src, edit)) - float(both.sum())) <= 1e-5 * float(both.sum())
    # antialias=False is a different table, hence another value, at a size that is resampled
    other = DinoModel("synthetic", "cpu", "tiny/8", antialias=False)
    assert abs(float(dino_structure(edit, src, other)[0]) - float(both[0])) > 1e-6


def test_cpu_float32_path_against_float64():
    from metrics import DinoModel, dino_structure
    for case in ("a20", "a64"):
        sd, x, b = dr.case_inputs(case)
        model = DinoModel(sd, "cpu")
        assert (model.patch, model.image, model.width) == (8, 32, 128) and model.backend.depth == 3
        k64 = dr.image_keys(sd, x, -1, 1)
        s64 = dr.score(k64[:b], k64[b:])
        keys = model.keys(x)
        got = dino_structure(x[b:], x[:b], model)
        rel = ((got - s64).abs() / s64).max().item()
        print(f"dino cpu float32 {case}: keys max |diff| {(keys.double() - k64).abs().max():.3e}, score rel {rel:.3e}")
        assert keys.shape == k64.shape == (2 * b, 17, 128) and keys.dtype == torch.float32
        assert rel <= 1e-4


def test_compute_metrics_cli_with_dino_weights(tmp_path):
    import yaml
    import compute_metrics
    from metrics import DinoModel, dino_structure
    from modules.models import StablePreprocess
    root, out, stems, prompts, files = _sweep(tmp_path)
    args = ["--data_path", str(root), "--output", str(out), "--device", "cpu", "--size", "32", "--batch", "3", "--limit", "4"]
    with pytest.raises(NotImplementedError, match="pretrained CLIP / DINO / LPIPS weights"):
        compute_metrics.main(args + ["--metric", "dinovitstruct"])
    assert not list((out / "metrics").glob("*.yaml")) if (out / "metrics").exists() else True
    a = compute_metrics.parse_args(args + ["--dino_weights", "w.pth"])
    assert (a.dino_weights, a.dino_model) == ("w.pth", "dino_vitb8")
    compute_metrics.main(args + ["--metric", "dinovitstruct", "mse", "--dino_weights", "synthetic", "--dino_model", "tiny/8"])
    assert sorted(f.name for f in (out / "metrics").glob("*.yaml")) == ["dinovitstruct.yaml", "mse.yaml"]
    pre = StablePreprocess("cpu", size=32, center_crop=True)
    model = DinoModel("synthetic", "cpu", "tiny/8")
    edits, sources = torch.cat([pre(out / "imgs" / f"{s}.png") for s in stems]), torch.cat([pre(f) for f in files])
    want = torch.cat([dino_structure(edits[:3], sources[:3], model), dino_structure(edits[3:], sources[3:], model)])
    res = yaml.safe_load((out / "metrics" / "dinovitstruct.yaml").read_text())
    assert set(res) == {"name", "mean", "results"} and res["name"] == "dinovitstruct"
    assert [r["file"] for r in res["results"]] == stems and all(set(r) == {"value", "file"} for r in res["results"])
    vals = [r["value"] for r in res["results"]]
    assert all(isinstance(v, float) and math.isfinite(v) and v > 0 for v in vals) and res["mean"] == float(np.mean(vals))
    assert vals == [float(v) for v in want]                           # the same batches of 3 + 1
