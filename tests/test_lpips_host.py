"""CPU-only checks of the lpips / bglpips metrics' host side: the C ABI's declarations and refusals, the weight loader, what the model, the classes
and EditMetric build and refuse, the CPU float32 path against float64, and compute_metrics.py on a four-image sweep with masks."""
import ctypes
import inspect
import math

import numpy as np
import pytest
import torch

from tests import lpips_ref as lr
from tests.test_clip_host import ROOT, _sweep

NEW_SYMBOLS = ["etainv_lpips_preprocess", "etainv_op_conv2d_relu", "etainv_op_maxpool3s2", "etainv_lpips_layer_distance"]
OLD_REFUSAL = ("metric '%s' is not built: built are ssim, msssim, mse, psnr; the others (clip_text_img, clip_img_img, clip_text_text, "
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
    assert "int64_t etainv_lpips_distance_workspace_bytes(int b, int pixels);" in header and hasattr(lib, "etainv_lpips_distance_workspace_bytes")
    assert _capi._RESTYPES["etainv_lpips_distance_workspace_bytes"] is ctypes.c_int64
    for cited in ("metrics/metrics.py:40-61", "metrics/bglpips.py:27-52", ":141-148"):
        assert cited in header, cited
    assert "lpips" in (ROOT / "eta-inversion_amd" / "csrc" / "build.sh").read_text().split("SRCS=")[1].split('"')[1].split()


def test_abi_refusals_by_message():
    from etainv import _capi
    lib = _capi.load()
    p = 0x10000                       # a stand-in pointer: every refusal below is made before anything touches the device
    err = lambda: lib.etainv_last_error().decode()
    call = lambda fn, order, base: (lambda **k: fn(*[{**base, **k}[n] for n in order]))
    pre = call(lib.etainv_lpips_preprocess, ("x", "mask", "n", "nm", "h", "w", "lo", "hi", "out", "dt", "st"),
               dict(x=p, mask=None, n=2, nm=0, h=31, w=31, lo=-1.0, hi=1.0, out=p, dt=_capi.F16, st=None))
    assert pre(x=None) != 0 and "null pointer" in err() and "etainv_lpips_preprocess" in err()
    assert pre(out=None) != 0 and "null pointer" in err()
    assert pre(out=p + 8) != 0 and "aligned" in err()
    assert pre(x=p + 2) != 0 and "aligned" in err()
    assert pre(mask=p, nm=0) != 0 and "n_mask" in err()
    assert pre(lo=1.0) != 0 and "hi > lo" in err()
    assert pre(h=0) != 0 and "16384" in err()
    assert pre(dt=9) != 0 and "bad dtype" in err()
    assert pre(n=0) == 0 and pre(n=0, nm=-5) == 0                      # a null mask ignores n_mask; nothing is launched for n = 0
    conv = call(lib.etainv_op_conv2d_relu, ("x", "w", "bias", "out", "n", "h", "wd", "cin", "cout", "kh", "kw", "stride", "pad", "relu", "dt", "st"),
                dict(x=p, w=p, bias=p, out=p, n=2, h=31, wd=31, cin=4, cout=64, kh=11, kw=11, stride=4, pad=2, relu=1, dt=_capi.F16, st=None))
    assert conv(x=None) != 0 and "null pointer" in err() and "etainv_op_conv2d_relu" in err()
    assert conv(w=None) != 0 and "null pointer" in err()
    assert conv(out=None) != 0 and "null pointer" in err()
    assert conv(x=p + 8) != 0 and "16-byte aligned" in err()
    assert conv(out=p + 4) != 0 and "16-byte aligned" in err()
    assert conv(bias=p + 2) != 0 and "aligned" in err()
    assert conv(h=6) != 0 and "smaller than 1 x 1" in err()            # 6 + 2 * 2 < 11
    assert conv(wd=6) != 0 and "smaller than 1 x 1" in err()
    assert conv(cin=3) != 0 and "cin must be 4" in err()
    assert conv(cin=48) != 0 and "multiple of 32" in err()
    assert conv(cout=30) != 0 and "cout must be a multiple of 4" in err()
    assert conv(kh=12) != 0 and "[1, 11]" in err()
    assert conv(stride=2) != 0 and "stride must be 1 or 4" in err()
    assert conv(pad=3) != 0 and "pad must be in [0, 2]" in err()
    assert conv(dt=5) != 0 and "bad dtype" in err()
    assert conv(n=0) == 0 and conv(n=0, bias=None, h=7, wd=7) == 0     # 7 + 4 = 11: one output pixel
    pool = call(lib.etainv_op_maxpool3s2, ("x", "out", "n", "h", "w", "c", "dt", "st"), dict(x=p, out=p, n=2, h=7, w=7, c=64, dt=_capi.F16, st=None))
    assert pool(x=None) != 0 and "null pointer" in err() and "etainv_op_maxpool3s2" in err()
    assert pool(out=p + 8) != 0 and "16-byte aligned" in err()
    assert pool(h=2) != 0 and "window of 3" in err()
    assert pool(c=12) != 0 and "16-byte vectors" in err()
    assert pool(c=12, dt=_capi.F32, n=0) == 0 and pool(n=0) == 0
    ws = lib.etainv_lpips_distance_workspace_bytes
    assert ws(1, 1) == 8 and ws(3, 225) == 3 * 4 * 8 and ws(32, 127 * 127) == 32 * 253 * 8 and ws(0, 9) == 0
    assert ws(1, 0) == -1 and "pixels in [1, 2^24]" in err()
    assert ws(40000, 4) == -1 and "32767" in err()
    dist = call(lib.etainv_lpips_layer_distance, ("f", "w", "b", "px", "c", "acc", "out", "ws", "bytes", "dt", "st"),
                dict(f=p, w=p, b=1, px=9, c=64, acc=0, out=p, ws=p, bytes=1 << 16, dt=_capi.F16, st=None))
    assert dist(f=None) != 0 and "null pointer" in err() and "etainv_lpips_layer_distance" in err()
    assert dist(w=None) != 0 and "null pointer" in err()
    assert dist(out=None) != 0 and "null pointer" in err()
    assert dist(ws=None) != 0 and "null pointer" in err()
    assert dist(f=p + 2) != 0 and "aligned" in err()
    assert dist(out=p + 4) != 0 and "8-byte aligned" in err()
    assert dist(px=0) != 0 and "pixels" in err()
    assert dist(c=0) != 0 and "c must be" in err()
    assert dist(acc=2) != 0 and "accumulate" in err()
    assert dist(bytes=4) != 0 and "workspace too small" in err()
    assert dist(dt=7) != 0 and "bad dtype" in err()
    assert dist(b=0) == 0


def test_weight_loader_takes_every_form_and_refuses_by_name(tmp_path):
    from etainv.weights import LPIPS_WIDTHS, load_lpips_state_dict, lpips_shapes, synthetic_lpips_state_dict
    sd = synthetic_lpips_state_dict(seed=1, net="tiny")
    assert LPIPS_WIDTHS == {"alex": (64, 192, 384, 256, 256), "tiny": (16, 32, 48, 32, 32)}
    assert {k: tuple(v.shape) for k, v in sd.items()} == lpips_shapes(LPIPS_WIDTHS["tiny"])
    assert sd["features.0.weight"].shape == (16, 3, 11, 11) and sd["features.3.weight"].shape == (32, 16, 5, 5) and sd["lin2.model.1.weight"].shape == (1, 48, 1, 1)
    again = synthetic_lpips_state_dict(seed=1, net="tiny")
    assert all(torch.equal(sd[k], again[k]) for k in sd) and not torch.equal(sd["features.0.weight"], synthetic_lpips_state_dict(seed=2, net="tiny")["features.0.weight"])
    for i in range(5):
        lin = sd[f"lin{i}.model.1.weight"]
        assert lin.min() >= 0 and 0.5 / lin.shape[1] < float(lin.mean()) < 4.0 / lin.shape[1]
    assert (sd["features.3.bias"] > 0).any() and (sd["features.3.bias"] < 0).any() and sd["features.3.bias"].abs().max() < 0.5
    assert 0.7 < float(sd["features.6.weight"].std()) / math.sqrt(2.0 / (32 * 9)) < 1.3                                   # He scaling
    full = synthetic_lpips_state_dict(net="alex")
    assert full["features.0.weight"].shape == (64, 3, 11, 11) and full["features.10.weight"].shape == (256, 256, 3, 3) and full["lin1.model.1.weight"].shape == (1, 192, 1, 1)
    with pytest.raises(ValueError, match="alex, tiny"):
        synthetic_lpips_state_dict(net="vgg")
    slice_of = {0: 1, 3: 2, 6: 3, 8: 4, 10: 5}
    conv_items = [(k, v) for k, v in sd.items() if k.startswith("features.")]
    lin_items = [(k, v) for k, v in sd.items() if k.startswith("lin")]
    lpips_form = {f"net.slice{slice_of[int(k.split('.')[1])]}.{k.split('.', 1)[1]}": v for k, v in conv_items}
    lpips_form.update({k: v for k, v in lin_items})
    lpips_form.update({k.replace("lin", "lins.", 1): v for k, v in lin_items})
    lpips_form["scaling_layer.shift"] = torch.tensor(lr.SHIFT).view(1, 3, 1, 1)
    lpips_form["scaling_layer.scale"] = torch.tensor(lr.SCALE).view(1, 3, 1, 1)
    lins_only = {"module." + k.replace("lin", "lins.", 1): v.half() for k, v in lin_items}
    backbone = {**dict(conv_items), "classifier.1.weight": torch.zeros(4, 4), "classifier.1.bias": torch.zeros(4)}
    heads = dict(lin_items)
    for form in (lpips_form, {k: v for k, v in lpips_form.items() if not k.startswith("lin") or k.startswith("lins.")}, {**backbone, **heads}, sd, {"state_dict": sd}):
        f = tmp_path / "w.pth"
        torch.save(form, f)
        got = load_lpips_state_dict(f)
        assert set(got) == set(sd) and all(torch.equal(got[k], sd[k]) and got[k].dtype == torch.float32 for k in sd)
        assert set(load_lpips_state_dict(form)) == set(sd)
    fb, fh = tmp_path / "backbone.pth", tmp_path / "heads.pth"
    torch.save(backbone, fb)
    torch.save(lins_only, fh)
    got = load_lpips_state_dict((fb, fh))
    assert set(got) == set(sd) and torch.equal(got["lin3.model.1.weight"], sd["lin3.model.1.weight"].half().float())
    assert torch.equal(load_lpips_state_dict([backbone, heads])["features.8.bias"], sd["features.8.bias"])
    with pytest.raises(ValueError, match="lin2.model.1.weight missing"):
        load_lpips_state_dict({k: v for k, v in sd.items() if k != "lin2.model.1.weight"})
    with pytest.raises(ValueError, match="features.6.weight missing"):
        load_lpips_state_dict({k: v for k, v in sd.items() if k != "features.6.weight"})
    with pytest.raises(ValueError, match="features.8.bias missing"):
        load_lpips_state_dict({k: v for k, v in lpips_form.items() if k != "net.slice4.8.bias"})
    with pytest.raises(ValueError, match=r"features.3.weight has shape \(32, 16, 3, 3\)"):
        load_lpips_state_dict({**sd, "features.3.weight": torch.zeros(32, 16, 3, 3)})
    with pytest.raises(ValueError, match="lin0.model.1.weight has shape"):
        load_lpips_state_dict({**sd, "lin0.model.1.weight": torch.zeros(1, 17, 1, 1)})
    with pytest.raises(ValueError, match="scaling_layer.shift"):
        load_lpips_state_dict({**lpips_form, "scaling_layer.shift": torch.tensor([-.03, -.088, -.2]).view(1, 3, 1, 1)})
    with pytest.raises(ValueError, match="scaling_layer.scale"):
        load_lpips_state_dict({**lpips_form, "scaling_layer.scale": torch.tensor([.458, .448, .5]).view(1, 3, 1, 1)})
    with pytest.raises(ValueError, match="not an LPIPS state dict"):
        load_lpips_state_dict({"blocks.0.attn.qkv.weight": torch.zeros(1)})
    assert "not verified" in load_lpips_state_dict.__doc__.lower()


def test_class_surface_reprs_and_refusals():
    import metrics
    from metrics import BGLPIPS, EditMetric, LPIPSMetric, LpipsModel, SimpleMetric, lpips_distance
    assert all(n in metrics.__all__ for n in ("LPIPSMetric", "BGLPIPS", "LpipsModel", "lpips_distance"))
    par = inspect.signature(LpipsModel.__init__).parameters
    assert list(par) == ["self", "weights", "device", "net", "compute_dtype", "seed"]
    assert (par["net"].default, par["compute_dtype"].default, par["seed"].default) == ("alex", torch.float16, 0)
    assert list(inspect.signature(lpips_distance).parameters) == ["edit", "source", "model", "input_range", "mask"]
    assert list(inspect.signature(LPIPSMetric.forward).parameters) == ["self", "pred", "target"]
    assert list(inspect.signature(BGLPIPS.forward).parameters) == ["self", "source_image", "target_image", "prompt", "mask"]
    assert issubclass(LPIPSMetric, SimpleMetric) and issubclass(BGLPIPS, SimpleMetric)
    model = LpipsModel("synthetic", "cpu", "tiny")
    assert model.widths == (16, 32, 48, 32, 32) and model.dtype == torch.float32 and model.device == "cpu"
    assert LpipsModel(model, "cpu").backend is model.backend                                       # a loaded model is shared
    assert repr(LPIPSMetric(device="cpu", weights=model)) == "lpips" and repr(BGLPIPS(device="cpu", weights=model)) == "bglpips"
    assert repr(EditMetric("lpips", device="cpu", lpips_weights=model)) == "lpips"
    assert repr(EditMetric("bglpips", device="cpu", lpips_weights="synthetic", lpips_net="tiny")) == "bglpips"
    assert EditMetric.get_built_metrics() == ["ssim", "msssim", "mse", "psnr"] and len(EditMetric.get_available_metrics()) == 14
    with pytest.raises(ValueError, match="weights="):
        LPIPSMetric(device="cpu")
    with pytest.raises(ValueError, match="weights="):
        BGLPIPS(device="cpu")
    with pytest.raises(NotImplementedError, match="net='alex'"):
        LpipsModel("synthetic", "cpu", "vgg")
    z = torch.zeros(1, 3, 30, 64)
    with pytest.raises(ValueError, match="at least 31 x 31"):
        lpips_distance(z, z, model)
    with pytest.raises(ValueError, match="at least 31 x 31"):
        lpips_distance(z.transpose(2, 3), z.transpose(2, 3), model)
    with pytest.raises(ValueError, match="same dimensions"):
        lpips_distance(torch.zeros(1, 3, 32, 32), torch.zeros(1, 3, 40, 40), model)
    with pytest.raises(ValueError, match=r"\(B, 3, H, W\)"):
        lpips_distance(torch.zeros(1, 4, 32, 32), torch.zeros(1, 4, 32, 32), model)
    with pytest.raises(ValueError, match="the mask must be"):
        lpips_distance(torch.zeros(2, 3, 32, 32), torch.zeros(2, 3, 32, 32), model, mask=torch.zeros(3, 32, 32))
    with pytest.raises(ValueError, match="float32"):
        lpips_distance(torch.zeros(2, 3, 32, 32), torch.zeros(2, 3, 32, 32), model, mask=torch.zeros(32, 32, dtype=torch.float64))
    for name in ("lpips", "bglpips"):                                                              # without lpips_weights: word for word as before
        for kw in ({}, {"clip_weights": "synthetic"}, {"dino_weights": "synthetic"}):
            with pytest.raises(NotImplementedError) as e:
                EditMetric(name, **kw)
            assert str(e.value) == OLD_REFUSAL % name
    with pytest.raises(NotImplementedError) as e:
        EditMetric("nslpips")
    assert str(e.value) == OLD_REFUSAL % "nslpips"
    with pytest.raises(NotImplementedError) as e:
        EditMetric("nslpips", lpips_weights="synthetic")
    assert all(w in str(e.value) for w in ("nslpips", "inversion", "attention store"))
    with pytest.raises(NotImplementedError, match="pretrained CLIP / DINO / LPIPS weights"):
        EditMetric("dinovitstruct", lpips_weights="synthetic")
    with pytest.raises(NotImplementedError, match="pretrained CLIP / DINO / LPIPS weights"):
        EditMetric("clip_text_text", lpips_weights="synthetic")


def test_edit_metric_argument_order_none_mask_and_batches():
    from metrics import EditMetric, LpipsModel, lpips_distance
    model = LpipsModel("synthetic", "cpu", "tiny")
    src, edit = lr.make_images(2, 40, 44, seed=9)
    mask = lr.make_masks(2, 40, 44, seed=10)
    both = lpips_distance(edit, src, model)
    bg = lpips_distance(edit, src, model, mask=mask)
    assert both.shape == (2,) and both.dtype == torch.float64 and (both > 0).all() and (bg > 0).all() and not torch.equal(bg, both)
    m = EditMetric("lpips", device="cpu", lpips_weights=model)
    seen = []
    inner = m.metric.forward
    m.metric.forward = lambda *a: (seen.append(a), inner(*a))[1]
    vals = [m.update(src[i:i + 1], edit[i:i + 1], "a cat", "a dog", "dog") for i in range(2)]
    assert all(isinstance(v, float) for v in vals) and len(seen[0]) == 2
    assert torch.equal(seen[0][0], src[:1]) and torch.equal(seen[0][1], edit[:1])                  # (source_image, edit_image)
    assert vals == [float(lpips_distance(edit[i:i + 1], src[i:i + 1], model)[0]) for i in range(2)] and np.allclose(vals, both.numpy(), rtol=1e-5)
    mean, info = m.compute()
    assert mean == float(np.mean(vals)) and info["all"] == vals
    b = EditMetric("bglpips", device="cpu", lpips_weights=model)
    seen.clear()
    inner_b = b.metric.forward
    b.metric.forward = lambda *a: (seen.append(a), inner_b(*a))[1]
    got = [b.update(src[i:i + 1], edit[i:i + 1], "a cat", "a dog", "dog", mask[i]) for i in range(2)]
    assert len(seen[0]) == 4 and torch.equal(seen[0][0], src[:1]) and torch.equal(seen[0][1], edit[:1]) and seen[0][2] == "a cat" and torch.equal(seen[0][3], mask[0])
    assert np.allclose(got, bg.numpy(), rtol=1e-5) and got == [float(lpips_distance(edit[i:i + 1], src[i:i + 1], model, mask=mask[i:i + 1])[0]) for i in range(2)]
    assert b.update(src[:1], edit[:1], "a cat", "a dog", "dog", None) is None and b.update(src[:1], edit[:1], "a cat", "a dog", "dog") is None
    assert b.metric.losses == got                                                                  # a None mask records nothing
    assert b.update(src[:1], edit[:1], "a cat", "a dog", "dog", mask[0][None]) == got[0]           # (1, H, W)
    assert b.update(src[:1], edit[:1], "a cat", "a dog", "dog", mask[0].numpy()) == got[0]         # an ndarray, as the reference takes
    # a batch handed to the class gives (B, 1, 1, 1), as lpips.LPIPS does
    out = m.metric(src, edit)
    assert out.shape == (2, 1, 1, 1) and torch.equal(out.flatten(), both)
    assert b.metric(src, edit, "", mask).shape == (2, 1, 1, 1) and b.metric(src[0], edit[0], "", mask[0]).shape == (1, 1, 1, 1)
    # identical images: exactly 0; a full-foreground mask: exactly 0; swapping the sides changes nothing
    assert float(lpips_distance(src, src, model).abs().max()) == 0.0
    assert float(lpips_distance(edit, src, model, mask=torch.ones(40, 44)).abs().max()) == 0.0
    assert torch.equal(lpips_distance(src, edit, model, mask=mask), bg)
    assert torch.allclose(lpips_distance(edit * 127.5 + 127.5, src * 127.5 + 127.5, model, input_range=(0, 255)), both, rtol=1e-4, atol=0)


@pytest.mark.parametrize("case", ["s64", "m67"])
def test_cpu_float32_path_against_float64(case):
    from metrics import LpipsModel, lpips_distance
    from metrics.lpips import lpips_taps
    sd = lr.model_state_dict()
    model = LpipsModel(sd, "cpu")
    assert model.widths == (64, 192, 384, 256, 256)
    x, b, mask = lr.case_inputs(case)
    s64, t64 = lr.score(sd, x, b, -1, 1, mask)
    got = lpips_distance(x[b:], x[:b], model, mask=mask)
    taps = lpips_taps(x, model, mask=mask)
    rel = ((got - s64).abs() / s64).max().item()
    err = max(float((t.double() - f.flatten(2).transpose(1, 2)).abs().max()) for t, f in zip(taps, t64))
    print(f"lpips cpu float32 {case}: taps max |diff| {err:.3e}, score rel {rel:.3e}")
    assert all(t.dtype == torch.float32 and t.shape == (2 * b, f.shape[2] * f.shape[3], f.shape[1]) for t, f in zip(taps, t64))
    assert got.dtype == torch.float64 and rel <= 1e-5 and err <= 1e-4


def test_compute_metrics_cli_with_lpips_weights(tmp_path):
    import yaml
    import compute_metrics
    from dataset.pie_bench_data import PieBenchData
    from metrics import LpipsModel, lpips_distance
    from modules.models import StablePreprocess
    root, out, stems, prompts, files = _sweep(tmp_path)
    args = ["--data_path", str(root), "--output", str(out), "--device", "cpu", "--batch", "3", "--limit", "4"]
    with pytest.raises(NotImplementedError, match="pretrained CLIP / DINO / LPIPS weights"):
        compute_metrics.main(args + ["--metric", "lpips"])
    a = compute_metrics.parse_args(args + ["--lpips_weights", "a.pth,b.pth"])
    assert (a.lpips_weights, a.lpips_net, a.size) == ("a.pth,b.pth", "alex", 512)
    with pytest.raises(ValueError, match="512 x 512 foreground masks"):
        compute_metrics.main(args + ["--metric", "lpips", "bglpips", "--lpips_weights", "synthetic", "--lpips_net", "tiny", "--size", "64"])
    assert not list((out / "metrics").glob("*.yaml")) if (out / "metrics").exists() else True     # refused before any yaml is claimed
    compute_metrics.main(args + ["--metric", "lpips", "bglpips", "mse", "--lpips_weights", "synthetic", "--lpips_net", "tiny"])
    assert sorted(f.name for f in (out / "metrics").glob("*.yaml")) == ["bglpips.yaml", "lpips.yaml", "mse.yaml"]
    pre = StablePreprocess("cpu", size=512, center_crop=True)
    model = LpipsModel("synthetic", "cpu", "tiny")
    data = PieBenchData(str(root), skip_img_load=True, limit=4)
    masks = torch.stack([data[i]["mask"] for i in range(4)])
    assert masks.shape == (4, 512, 512) and 0 < float(masks.mean()) < 1
    edits, sources = torch.cat([pre(out / "imgs" / f"{s}.png") for s in stems]), torch.cat([pre(f) for f in files])
    for name, mk in (("lpips", None), ("bglpips", masks)):
        want = torch.cat([lpips_distance(edits[:3], sources[:3], model, mask=None if mk is None else mk[:3]),
                          lpips_distance(edits[3:], sources[3:], model, mask=None if mk is None else mk[3:])])
        res = yaml.safe_load((out / "metrics" / f"{name}.yaml").read_text())
        assert set(res) == {"name", "mean", "results"} and res["name"] == name
        assert [r["file"] for r in res["results"]] == stems and all(set(r) == {"value", "file"} for r in res["results"])
        vals = [r["value"] for r in res["results"]]
        assert all(isinstance(v, float) and math.isfinite(v) and v > 0 for v in vals) and res["mean"] == float(np.mean(vals))
        assert vals == [float(v) for v in want], name                 # the same batches of 3 + 1
    lp, bg = (yaml.safe_load((out / "metrics" / f"{n}.yaml").read_text())["results"] for n in ("lpips", "bglpips"))
    assert all(a["value"] != b["value"] for a, b in zip(lp, bg))
