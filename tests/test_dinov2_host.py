"""CPU-only checks of the dinovitstruct_v2 metric's host side: the C ABI's declarations and refusals, the weight loader, dinov2_geometry and the
position table the library builds, what Dinov2Model and EditMetric build and refuse (every refusal that was there before included), the CPU
float32 path against float64, and compute_metrics.py on a four-image sweep."""
import ctypes
import inspect
import math

import numpy as np
import pytest
import torch

from tests import dinov2_ref as v2
from tests.test_clip_host import ROOT, _sweep
from tests.test_dino_host import OLD_REFUSAL

NEW_SYMBOLS = ["etainv_dinov2_preprocess", "etainv_op_layerscale_add_layernorm"]


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
    assert "#define ETAINV_DINOV2_KP 640" in header
    for cited in ("dino_vit_structure.py:32-34", ":120-122", ":141-160"):
        assert cited in header, cited


def test_abi_refusals_by_message():
    from etainv import _capi
    lib = _capi.load()
    p = 0x10000                       # a stand-in pointer: every refusal below is made before anything touches the device
    err = lambda: lib.etainv_last_error().decode()
    order = ("x", "b", "s", "r", "lo", "hi", "bh", "ch", "kh", "bv", "cv", "kv", "rows", "out", "dt", "st")
    pre = lambda **k: lib.etainv_dinov2_preprocess(*[{**dict(x=p, b=1, s=512, r=224, lo=-1.0, hi=1.0, bh=p, ch=p, kh=5, bv=p, cv=p, kv=5, rows=37,
                                                           out=p, dt=_capi.F16, st=None), **k}[n] for n in order])
    assert pre(x=None) != 0 and "null pointer" in err() and "etainv_dinov2_preprocess" in err()
    assert pre(out=None) != 0 and "null pointer" in err()
    assert pre(cv=None) != 0 and "null pointer" in err()
    assert pre(out=p + 2) != 0 and "aligned" in err()
    assert pre(bh=p + 1) != 0 and "aligned" in err()
    assert pre(r=220) != 0 and "multiple of the patch size" in err()
    assert pre(r=0) != 0 and "multiple of the patch size" in err()
    assert pre(b=65536) != 0 and "65535" in err()
    assert pre(hi=-1.0) != 0 and "hi > lo" in err()
    assert pre(s=4096, rows=400) != 0 and "LDS" in err()
    assert pre(dt=7) != 0 and "bad dtype" in err()
    assert pre(b=0) == 0                                              # 512 -> 224 at p = 14 (37 rows of 224 floats) fits; nothing is launched for b = 0
    order = ("y", "ls", "x", "g", "be", "eps", "xo", "ho", "rows", "c", "dt", "st")
    fus = lambda **k: lib.etainv_op_layerscale_add_layernorm(*[{**dict(y=p, ls=p + 0x100, x=p + 0x200, g=p + 0x300, be=p + 0x400, eps=1e-6, xo=p + 0x500,
                                                                     ho=p + 0x600, rows=0, c=768, dt=_capi.F16, st=None), **k}[n] for n in order])
    for name in ("y", "ls", "x", "g", "be", "ho"):
        assert fus(**{name: None}) != 0 and "null pointer" in err() and "etainv_op_layerscale_add_layernorm" in err(), name
    for c in (0, 4, 100, 1544, 2048):
        assert fus(c=c) != 0 and "multiple of 8 and at most 1536" in err(), c
    for name in ("y", "x", "xo", "ho", "ls"):
        assert fus(**{name: p + 0x708}) != 0 and "16-byte aligned" in err(), name
    assert fus(g=p + 2) != 0 and "aligned" in err()
    assert fus(dt=9) != 0 and "bad dtype" in err()
    assert fus(rows=-1) != 0 and "rows" in err()
    assert fus(ho=p + 0x200) != 0 and "buffer of its own" in err()       # h_out == x
    assert fus() == 0 and fus(xo=None) == 0 and fus(xo=p + 0x200) == 0 and fus(c=1536, dt=_capi.F32) == 0 and fus(c=8, dt=_capi.BF16) == 0    # rows = 0


def test_weight_loader_unwraps_strips_and_refuses(tmp_path):
    from etainv.nets import dino_geometry, dinov2_geometry
    from etainv.weights import load_dino_state_dict, load_dinov2_state_dict, synthetic_dino_state_dict, synthetic_dinov2_state_dict
    sd = synthetic_dinov2_state_dict(width=128, layers=2, patch=14, image=42, table=5, seed=1)
    assert sd["pos_embed"].shape == (1, 26, 128) and sd["patch_embed.proj.weight"].shape == (128, 3, 14, 14) and sd["blocks.1.ls2.gamma"].shape == (128,)
    again = synthetic_dinov2_state_dict(width=128, layers=2, patch=14, image=42, table=5, seed=1)
    assert all(torch.equal(sd[k], again[k]) for k in sd)
    gam = torch.cat([sd[f"blocks.{i}.{n}.gamma"] for i in range(2) for n in ("ls1", "ls2")])
    assert gam.abs().min() >= 1e-5 * (1 - 1e-6) and gam.abs().max() <= 1 and gam.abs().min() < 1e-4 and gam.abs().max() > 0.1 and (gam < 0).any() and (gam > 0).any()
    wrapped = {"teacher": {"module.backbone." + k: v.half() for k, v in sd.items()}, "student": {}, "epoch": 3}
    wrapped["teacher"]["module.head.last_layer.weight"] = torch.zeros(4, 4)
    for form in (wrapped, {"state_dict": {"backbone." + k: v for k, v in sd.items()}}, sd):
        f = tmp_path / "w.pth"
        torch.save(form, f)
        got = load_dinov2_state_dict(f)
        assert set(got) == set(sd) and all(v.dtype == torch.float32 for v in got.values())
        assert torch.equal(got["cls_token"], sd["cls_token"].half().float() if form is wrapped else sd["cls_token"])
    assert set(load_dinov2_state_dict({**sd, "head.weight": torch.zeros(3, 3)})) == set(sd)
    with pytest.raises(ValueError, match="register_tokens"):
        load_dinov2_state_dict({**sd, "register_tokens": torch.zeros(1, 4, 128)})
    with pytest.raises(ValueError, match="SwiGLU"):
        load_dinov2_state_dict({**sd, "blocks.0.mlp.w12.weight": torch.zeros(8, 128)})
    with pytest.raises(ValueError, match="blocks.0.ls1.gamma missing"):
        load_dinov2_state_dict(synthetic_dino_state_dict(width=128, layers=2, patch=8, image=32))
    # the DINO loader and geometry still refuse these weights, by the same words
    with pytest.raises(ValueError, match="DINOv2"):
        load_dino_state_dict(sd)
    with pytest.raises(ValueError, match="DINOv2"):
        dino_geometry(sd)
    # geometry
    assert dinov2_geometry(sd) == {"width": 128, "patch": 14, "layers": 2, "table": 5, "image": 70, "g2": 25}
    assert dinov2_geometry(sd, 42) == {"width": 128, "patch": 14, "layers": 2, "table": 5, "image": 42, "g2": 9}
    big = {**sd, "pos_embed": torch.zeros(1, 1370, 128)}
    assert dinov2_geometry(big)["image"] == 224 and dinov2_geometry(big)["g2"] == 256 and dinov2_geometry(big, 518)["g2"] == 1369
    with pytest.raises(ValueError, match="multiple of 64"):
        dinov2_geometry({**sd, "patch_embed.proj.weight": torch.zeros(96, 3, 14, 14)})
    with pytest.raises(ValueError, match="14 x 14"):
        dinov2_geometry({**sd, "patch_embed.proj.weight": torch.zeros(128, 3, 16, 16)})
    with pytest.raises(ValueError, match="square M x M"):
        dinov2_geometry({**sd, "pos_embed": torch.zeros(1, 27, 128)})
    with pytest.raises(ValueError, match="multiple of 14"):
        dinov2_geometry(sd, 40)
    with pytest.raises(ValueError, match="register"):
        dinov2_geometry({**sd, "register_tokens": torch.zeros(1, 4, 128)})
    with pytest.raises(ValueError, match="ls1.gamma missing"):
        dinov2_geometry({k: v for k, v in sd.items() if "ls1" not in k})


@pytest.mark.parametrize("offset", [0.1, 0.0])
@pytest.mark.parametrize("m,g", [(37, 16), (5, 3), (3, 4)])
def test_position_table_is_dinov2_refs(m, g, offset):
    """the library's table (F.interpolate in float32, the call the published model makes) against the float64 restatement, under the bound of
    tests/test_dinov2_ref.py for torch's float32 kernel"""
    from etainv.nets import dinov2_position_table
    pos = torch.randn(1, 1 + m * m, 16, generator=torch.Generator().manual_seed(g))
    got = dinov2_position_table(pos, g, offset)
    want = v2.position_table(pos, g, offset)
    assert got.dtype == torch.float32 and got.shape == want.shape and torch.equal(got[0], pos[0, 0])
    assert (got.double() - want).abs().max().item() <= (36 * m + 40) * 2.0 ** -24 * pos.abs().max().item()
    assert torch.equal(dinov2_position_table(pos, m, offset), pos[0])


def test_class_surface_reprs_and_refusals():
    from metrics import DinoModel, Dinov2Model, DinoVitStructure, EditMetric, dino_structure
    from metrics.dino_vit_structure import GEOMETRY_V2
    assert set(GEOMETRY_V2) == {"dinov2_vits14", "dinov2_vitb14", "dinov2_vitl14", "tinyv2/14"}
    assert GEOMETRY_V2["dinov2_vitb14"] == dict(width=768, layers=12, patch=14, image=224, table=37)
    assert GEOMETRY_V2["tinyv2/14"] == dict(width=128, layers=2, patch=14, image=42, table=5)
    par = inspect.signature(Dinov2Model.__init__).parameters
    assert list(par)[:8] == ["self", "weights", "device", "dino_model", "compute_dtype", "antialias", "interpolate_offset", "seed"]
    assert (par["dino_model"].default, par["compute_dtype"].default, par["antialias"].default, par["interpolate_offset"].default) == \
        ("dinov2_vitb14", torch.float16, True, 0.1)
    model = Dinov2Model("synthetic", "cpu", "tinyv2/14")
    assert (model.patch, model.image, model.width, model.table, model.antialias, model.interpolate_offset) == (14, 42, 128, 5, True, 0.1)
    assert model.backend.pos.shape == (10, 128)
    assert Dinov2Model(model, "cpu").backend is model.backend                                                 # a loaded model is shared
    assert repr(DinoVitStructure(device="cpu", vit_model="tinyv2/14", weights=model)) == "tinyv2/14"
    assert isinstance(DinoVitStructure(device="cpu", vit_model="dinov2_vitb14", weights=model).model, Dinov2Model)
    m = EditMetric("dinovitstruct_v2", device="cpu", dinov2_weights=model)
    assert repr(m) == "dinov2_vitb14" and m.metric.model.backend is model.backend
    m = EditMetric("dinovitstruct_v2", device="cpu", dinov2_weights="synthetic", dinov2_model="tinyv2/14")
    assert repr(m) == "tinyv2/14" and isinstance(m.metric.model, Dinov2Model)
    with pytest.raises(ValueError, match="weights="):
        DinoVitStructure(device="cpu", vit_model="dinov2_vitb14")
    with pytest.raises(ValueError, match="dino_model must be one of"):
        Dinov2Model("synthetic", "cpu", "dinov2_vitx14")
    with pytest.raises(NotImplementedError, match="SwiGLU"):
        Dinov2Model("synthetic", "cpu", "dinov2_vitg14")
    with pytest.raises(NotImplementedError, match="register"):
        Dinov2Model("synthetic", "cpu", "dinov2_vitb14_reg")
    with pytest.raises(ValueError, match="square"):
        model.keys(torch.zeros(1, 3, 42, 56))
    with pytest.raises(ValueError, match="square"):
        dino_structure(torch.zeros(1, 3, 42, 56), torch.zeros(1, 3, 42, 56), model)
    with pytest.raises(ValueError, match="same dimensions"):
        dino_structure(torch.zeros(1, 3, 32, 32), torch.zeros(1, 3, 40, 40), model)
    # everything that was refused before still is, by the same words
    assert EditMetric.get_built_metrics() == ["ssim", "msssim", "mse", "psnr"] and len(EditMetric.get_available_metrics()) == 14
    with pytest.raises(NotImplementedError, match="LayerScale"):
        DinoModel("synthetic", "cpu", "dinov2_vitb14")
    with pytest.raises(NotImplementedError) as e:
        EditMetric("dinovitstruct_v2")
    assert str(e.value) == OLD_REFUSAL.replace("metric 'dinovitstruct'", "metric 'dinovitstruct_v2'")
    with pytest.raises(NotImplementedError) as e:
        EditMetric("dinovitstruct_v2", dino_weights="synthetic")
    assert all(w in str(e.value) for w in ("patch 14", "LayerScale", "interpolated position embeddings", "pass dinov2_weights="))
    with pytest.raises(NotImplementedError, match="pretrained CLIP / DINO / LPIPS weights"):
        EditMetric("dinovitstruct", dinov2_weights="synthetic")
    with pytest.raises(NotImplementedError, match="pretrained CLIP / DINO / LPIPS weights"):
        EditMetric("lpips", dinov2_weights="synthetic")


def test_edit_metric_passes_source_then_edit_and_equals_dino_structure():
    from metrics import Dinov2Model, EditMetric, dino_structure
    model = Dinov2Model("synthetic", "cpu", "tinyv2/14")
    src, edit = v2.make_images(2, 40, -1, 1, seed=9)
    both = dino_structure(edit, src, model)
    assert both.shape == (2,) and both.dtype == torch.float64 and (both > 0).all()
    m = EditMetric("dinovitstruct_v2", device="cpu", dinov2_weights=model, dinov2_model="tinyv2/14")
    seen = []
    inner = m.metric.forward
    m.metric.forward = lambda pred, target: (seen.append((pred, target)), inner(pred, target))[1]
    vals = [m.update(src[i:i + 1], edit[i:i + 1], "a cat", "a dog", "dog") for i in range(2)]
    assert all(isinstance(v, float) for v in vals)
    assert torch.equal(seen[0][0], src[:1]) and torch.equal(seen[0][1], edit[:1])                             # (source_image, edit_image)
    alone = [float(dino_structure(src[i:i + 1], edit[i:i + 1], model)[0]) for i in range(2)]
    assert vals == alone and np.allclose(vals, both.numpy(), rtol=1e-5)
    mean, info = m.compute()
    assert mean == float(np.mean(vals)) and info["all"] == vals
    assert float(dino_structure(edit, edit, model).abs().max()) == 0.0
    # the other form of the position table is another model, hence another value
    other = Dinov2Model("synthetic", "cpu", "tinyv2/14", interpolate_offset=0.0)
    assert (other.backend.pos - model.backend.pos).abs().max() > 0.01
    assert abs(float(dino_structure(edit, src, other)[0]) - float(both[0])) > 1e-6


def test_cpu_float32_path_against_float64():
    from metrics import Dinov2Model, dino_structure
    for case in ("a20", "a64"):
        sd, image, x, b = v2.case_inputs(case)
        model = Dinov2Model(sd, "cpu", image=image)
        assert (model.patch, model.image, model.width, model.table) == (14, 42, 128, 5) and model.backend.depth == 3
        k64 = v2.image_keys(sd, x, -1, 1, image=image)
        s64 = v2.score(k64[:b], k64[b:])
        keys = model.keys(x)
        got = dino_structure(x[b:], x[:b], model)
        rel = ((got - s64).abs() / s64).max().item()
        print(f"dinov2 cpu float32 {case}: keys max |diff| {(keys.double() - k64).abs().max():.3e}, score rel {rel:.3e}")
        assert keys.shape == k64.shape == (2 * b, 10, 128) and keys.dtype == torch.float32
        assert rel <= 1e-4
    for offset in (0.1, 0.0):                                          # case B's 37 -> 16 table, both forms, two layers
        sd, image, x, b = v2.case_inputs("b")
        model = Dinov2Model(sd, "cpu", interpolate_offset=offset)
        keys = model.keys(x[:1])
        k64 = v2.image_keys(sd, x[:1], -1, 1, offset=offset)
        print(f"dinov2 cpu float32 b offset {offset}: keys max |diff| {(keys.double() - k64).abs().max():.3e}")
        assert keys.shape == (1, 257, 128) and model.image == 224 and (keys.double() - k64).abs().max() <= 1e-4


def test_compute_metrics_cli_with_dinov2_weights(tmp_path):
    import yaml
    import compute_metrics
    from metrics import Dinov2Model, dino_structure
    from modules.models import StablePreprocess
    root, out, stems, prompts, files = _sweep(tmp_path)
    args = ["--data_path", str(root), "--output", str(out), "--device", "cpu", "--size", "32", "--batch", "3", "--limit", "4"]
    with pytest.raises(NotImplementedError, match="pretrained CLIP / DINO / LPIPS weights"):
        compute_metrics.main(args + ["--metric", "dinovitstruct_v2"])
    assert not list((out / "metrics").glob("*.yaml")) if (out / "metrics").exists() else True
    a = compute_metrics.parse_args(args + ["--dinov2_weights", "w.pth"])
    assert (a.dinov2_weights, a.dinov2_model) == ("w.pth", "dinov2_vitb14")
    compute_metrics.main(args + ["--metric", "dinovitstruct_v2", "mse", "--dinov2_weights", "synthetic", "--dinov2_model", "tinyv2/14"])
    assert sorted(f.name for f in (out / "metrics").glob("*.yaml")) == ["dinovitstruct_v2.yaml", "mse.yaml"]
    pre = StablePreprocess("cpu", size=32, center_crop=True)
    model = Dinov2Model("synthetic", "cpu", "tinyv2/14")
    edits, sources = torch.cat([pre(out / "imgs" / f"{s}.png") for s in stems]), torch.cat([pre(f) for f in files])
    want = torch.cat([dino_structure(edits[:3], sources[:3], model), dino_structure(edits[3:], sources[3:], model)])
    res = yaml.safe_load((out / "metrics" / "dinovitstruct_v2.yaml").read_text())
    assert set(res) == {"name", "mean", "results"} and res["name"] == "dinovitstruct_v2"
    assert [r["file"] for r in res["results"]] == stems and all(set(r) == {"value", "file"} for r in res["results"])
    vals = [r["value"] for r in res["results"]]
    assert all(isinstance(v, float) and math.isfinite(v) and v > 0 for v in vals) and res["mean"] == float(np.mean(vals))
    assert vals == [float(v) for v in want]                           # the same batches of 3 + 1
