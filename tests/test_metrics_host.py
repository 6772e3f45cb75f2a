"""CPU-only checks of the metrics package and compute_metrics.py: the plain-torch float32 path of `image_metrics` against the reference's own
float32 values (tests/golden/metrics_ref.npz; bound: the fixture's yardstick, the largest |reference float32 - float64| per metric), the class
surface of the reference's metrics/ (names, repr, update / compute contract, refusals), the C ABI's refusals, and the command line over a
temporary sweep directory."""
import json
import math
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import metrics_ref as mr

GOLDEN = Path(__file__).resolve().parent / "golden"
NAMES14 = ["clip_text_img", "clip_img_img", "clip_text_text", "clip_textdir_imgdir", "clip_text_img_acc", "clip_text_text_acc", "dinovitstruct",
           "dinovitstruct_v2", "lpips", "bglpips", "ssim", "msssim", "mse", "psnr"]
BUILT = ["ssim", "msssim", "mse", "psnr"]


@pytest.fixture(scope="module")
def fixture():
    return np.load(GOLDEN / "metrics_ref.npz")


def names_for(h, w):
    return ("mse", "psnr", "ssim") + (("msssim",) if min(h, w) > 160 else ())


@pytest.mark.parametrize("case", mr.CASES, ids=[c[0] for c in mr.CASES])
def test_cpu_path_matches_reference_float32(fixture, case):
    from metrics import image_metrics
    name, h, w, _ = case
    pred, target = mr.make_pair(*case)
    got = image_metrics(pred[None], target[None], (-1, 1), names_for(h, w))
    for n, v in got.items():
        assert v.shape == (1,) and v.dtype == torch.float32
        yard, ref32 = float(fixture[f"yardstick/{n}"]), float(fixture[f"{name}/{n}/ref32"])
        print(f"{name} {n}: cpu path {v.item()!r} reference float32 {ref32!r} |diff| {abs(v.item() - ref32):.3g} yardstick {yard:.3g}")
        assert abs(v.item() - ref32) <= yard


def test_cpu_path_batch_rows_and_conversions():
    from metrics import image_metrics
    cases = [c for c in mr.CASES if c[1:3] == (161, 176)] + [("161x176b", 161, 176, 401), ("161x176c", 161, 176, 402)]
    pairs = [mr.make_pair(*c) for c in cases]
    pred, target = torch.stack([p for p, _ in pairs]), torch.stack([t for _, t in pairs])
    full = image_metrics(pred, target)
    assert list(full) == ["mse", "psnr", "ssim", "msssim"] and all(v.shape == (3,) for v in full.values())
    for i in range(3):
        one = image_metrics(pred[i:i + 1], target[i:i + 1])
        assert all(torch.equal(one[n][0], full[n][i]) for n in full)
    # float64 and non-contiguous inputs are converted; a [0, 1] input with input_range None is the same pair
    wide = image_metrics(pred.double().permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2), target.double(), which="ssim")
    assert list(wide) == ["ssim"] and torch.equal(wide["ssim"], full["ssim"])
    unit = image_metrics((pred + 1) / 2, (target + 1) / 2, None, ("mse",))
    assert torch.allclose(unit["mse"], full["mse"], rtol=1e-6, atol=0)


def test_window_constants():
    from metrics import functional as mf
    assert torch.equal(mf.gaussian_window(torch.float64), mr.window64())   # the constants are the float32 window torch builds, bit for bit
    assert torch.equal(mf.gaussian_window(), mr.window64().float())
    src = (Path(__file__).resolve().parents[1] / "eta-inversion_amd" / "csrc" / "metrics.hip").read_text()
    assert all(h + "f" in src for h in mf.WINDOW_HEX)                     # ... and the kernel holds the same ones


def test_refusals():
    from metrics import image_metrics
    a, b = torch.zeros(1, 3, 20, 20), torch.zeros(1, 3, 20, 21)
    with pytest.raises(ValueError, match=r"Input images should have the same dimensions, but got torch.Size\(\[1, 3, 20, 20\]\) and torch.Size\(\[1, 3, 20, 21\]\)\."):
        image_metrics(a, b)
    with pytest.raises(AssertionError, match="Image size should be larger than 160 due to the 4 downsamplings in ms-ssim"):
        image_metrics(torch.zeros(1, 3, 160, 200), torch.zeros(1, 3, 160, 200), which=("msssim",))
    with pytest.raises(ValueError, match="at least 11 x 11"):
        image_metrics(torch.zeros(1, 3, 10, 20), torch.zeros(1, 3, 10, 20), which=("ssim",))
    with pytest.raises(ValueError, match=r"\(B, 3, H, W\)"):
        image_metrics(torch.zeros(3, 20, 20), torch.zeros(3, 20, 20))
    with pytest.raises(ValueError, match="mse, psnr, ssim, msssim"):
        image_metrics(a, a, which=("lpips",))
    with pytest.raises(ValueError, match="hi > lo"):
        image_metrics(a, a, (1, 1), ("mse",))
    assert image_metrics(torch.zeros(2, 3, 5, 7), torch.ones(2, 3, 5, 7), (0, 1), ("mse", "psnr"))["mse"].tolist() == [1.0, 1.0]   # no window needed


def test_class_surface():
    import metrics
    from metrics import EditMetric
    from metrics.base import BaseMetric, SimpleMetric
    assert EditMetric.get_available_metrics() == NAMES14
    for name, cls in (("mse", metrics.MSEMetric), ("psnr", metrics.PSNRMetric), ("ssim", metrics.SSIM), ("msssim", metrics.MSSSIM)):
        m = cls(input_range=(-1, 1), device="cpu")
        assert repr(m) == name and isinstance(m, SimpleMetric) and issubclass(SimpleMetric, BaseMetric) and m.losses == []
        e = EditMetric(name, input_range=(-1, 1), device="cpu")
        assert repr(e) == name and str(e) == name and isinstance(e.metric, cls) and e.metric_name == name
    for name in [n for n in NAMES14 if n not in BUILT] + ["nslpips", "nonsense"]:
        with pytest.raises(NotImplementedError, match="ssim, msssim, mse, psnr") as err:
            EditMetric(name)
        assert "pretrained CLIP / DINO / LPIPS weights" in str(err.value)
    base = BaseMetric(input_range=(0, 255), device="cpu")
    assert torch.equal(base._normalize(torch.tensor([0.0, 51.0, 255.0])), torch.tensor([0.0, 0.2, 1.0]))
    x = torch.rand(3)
    assert BaseMetric(input_range=None, device="cpu")._normalize(x) is x
    for method in (base.forward, base.update, base.compute):
        with pytest.raises(NotImplementedError):
            method()
    assert BaseMetric().device == ("cuda" if torch.cuda.is_available() else "cpu")


def test_update_compute_contract():
    from metrics import MSEMetric, image_metrics
    pairs = [mr.make_pair("a", 12, 17, s) for s in (1, 2, 3)]
    m = MSEMetric(device="cpu")
    vals = [m.update(p[None], t[None]) for p, t in pairs]
    assert all(isinstance(v, float) for v in vals) and m.losses == vals
    assert vals == [image_metrics(p[None], t[None], which="mse")["mse"].item() for p, t in pairs]
    assert torch.equal(m(pairs[0][0][None], pairs[0][1][None]), image_metrics(pairs[0][0][None], pairs[0][1][None], which="mse")["mse"][0])   # a call records nothing
    mean, extra = m.compute()
    assert mean == float(np.mean(vals)) and isinstance(mean, float) and extra == {"value": mean, "all": vals}
    assert m.losses == []                                                  # compute forgets
    m.update(*[x[None] for x in pairs[0]])
    assert m.compute()[0] == vals[0]


def test_edit_metric_argument_order():
    from metrics import EditMetric
    source, edit = torch.rand(1, 3, 12, 12) * 2 - 1, torch.rand(1, 3, 12, 12) * 2 - 1
    for name in ("ssim", "mse", "psnr"):
        e = EditMetric(name, device="cpu")
        seen = []
        forward = e.metric.forward
        e.metric.forward = lambda *args: (seen.append(args), forward(*args))[1]
        v = e.update(source_image=source, edit_image=edit, source_prompt="a cat", target_prompt="a dog", edit_word="cat", mask=None)
        assert len(seen) == 1 and seen[0][0] is edit and seen[0][1] is source        # (pred, target) = (edit_image, source_image)
        assert isinstance(v, float) and e.compute() == (v, {"value": v, "all": [v]}) and e.metric.losses == []


def test_capi_symbol_and_refusals():
    from etainv import _capi
    lib = _capi.load()
    header = (Path(__file__).resolve().parents[1] / "include" / "etainv.h").read_text()
    for name, nargs in (("etainv_image_metrics", 12), ("etainv_image_metrics_workspace_bytes", 4)):
        assert f"{name}(" in header and len(_capi.SIGNATURES[name]) == nargs and hasattr(lib, name)
    assert lib.etainv_abi_version() == 1
    err = lambda: lib.etainv_last_error().decode()
    size = lib.etainv_image_metrics_workspace_bytes
    assert size(1, 11, 11, 4) > 0 and size(3, 512, 512, 15) > size(3, 512, 512, 7) > size(3, 512, 512, 3) > 0
    # five prep values per block (19 for 3 x 161 x 161 elements) and pair, three partial sums per tile of 16 x 32 window positions and plane, two float64 planes per pooled level
    assert size(1, 161, 161, 15) == 8 * (5 * 19 + 3 * 3 * (10 * 5 + 5 * 3 + 2 + 1 + 1) + 2 * 3 * (81 * 81 + 41 * 41 + 21 * 21 + 11 * 11))
    for args, fragment in (((1, 10, 20, 4), "h >= 11"), ((1, 160, 200, 8), "> 160"), ((1, 20, 20, 0), "mask"), ((1, 20, 20, 16), "mask"),
                           ((-1, 20, 20, 1), "negative"), ((1, 0, 20, 1), "[1, 16384]"), ((1, 20, 16385, 1), "[1, 16384]"), ((21846, 20, 20, 1), "21845")):
        assert size(*args) == -1 and fragment in err() and "etainv_image_metrics_workspace_bytes" in err(), (args, err())

    def call(**over):       # non-null stand-in pointers: a refused call never dereferences
        a = dict(pred=4096, target=8192, b=1, h=20, w=20, lo=-1.0, hi=1.0, mask=7, out=12288, ws=16384, ws_bytes=1 << 30)
        a.update(over)
        return lib.etainv_image_metrics(a["pred"], a["target"], a["b"], a["h"], a["w"], a["lo"], a["hi"], a["mask"], a["out"], a["ws"], a["ws_bytes"], None)
    for over, fragment in ((dict(pred=None), "null pointer"), (dict(target=None), "null pointer"), (dict(out=None), "null pointer"),
                           (dict(hi=-1.0), "hi > lo"), (dict(lo=float("nan")), "hi > lo"), (dict(hi=float("inf")), "hi > lo"),
                           (dict(ws=None), "workspace"), (dict(ws=16388), "8-byte aligned"), (dict(ws_bytes=64), "smaller than"),
                           (dict(h=10), "h >= 11"), (dict(mask=15), "> 160"), (dict(mask=32), "mask")):
        assert call(**over) != 0, over
        assert fragment in err() and "etainv_image_metrics" in err(), (over, err())
    assert call(b=0) == 0                                                  # nothing to do


# ---- compute_metrics.py
def _sweep(tmp_path, size=24):
    """a data set of four entries and the imgs/ directory an eval.py sweep leaves: pair 0 and 1 complete, 2 with an unreadable edited file,
    3 without its edited file"""
    from PIL import Image
    from dataset.pie_bench_data import edit_image_name
    g = json.loads((GOLDEN / "pie_bench.json").read_text())
    entries = list(g["mapping"].items())[:4]
    root, out = tmp_path / "pie", tmp_path / "res"
    (out / "imgs").mkdir(parents=True)
    rng = np.random.default_rng(0)
    stems = []
    for i, (key, e) in enumerate(entries):
        f = root / "annotation_images" / e["image_path"]
        f.parent.mkdir(parents=True, exist_ok=True)
        img = rng.integers(0, 256, (size, size + 6, 3), dtype=np.uint8)          # wider than high: the centre crop
        Image.fromarray(img).save(f)
        strip = lambda s: s.replace("[", "").replace("]", "")
        stems.append(edit_image_name(i, strip(e["original_prompt"]), strip(e["editing_prompt"])))
        if i < 2:
            Image.fromarray((img // 2 + rng.integers(0, 64, img.shape)).astype(np.uint8)).save(out / "imgs" / f"{stems[-1]}.png")
        elif i == 2:
            (out / "imgs" / f"{stems[-1]}.png").write_bytes(b"not a png")
    root.mkdir(exist_ok=True)
    (root / "mapping_file.json").write_text(json.dumps(dict(entries)))
    return root, out, stems


def test_compute_metrics_cli(tmp_path, capsys):
    import yaml
    import compute_metrics
    from metrics import image_metrics
    from modules.models import StablePreprocess
    root, out, stems = _sweep(tmp_path)
    (out / "metrics").mkdir()
    (out / "metrics" / "psnr.yaml").write_text("kept: true\n")                    # an existing yaml: that metric is skipped
    args = ["--data_path", str(root), "--output", str(out), "--device", "cpu", "--size", "24", "--batch", "2", "--limit", "4"]
    compute_metrics.main(args + ["--metric", "mse", "psnr", "ssim", "msssim"])
    printed = capsys.readouterr().out
    assert f"skipping {out / 'metrics' / 'psnr.yaml'}" in printed and f"Skipping {out / 'imgs' / (stems[3] + '.png')}" in printed
    assert (out / "metrics" / "psnr.yaml").read_text() == "kept: true\n"
    pre = StablePreprocess("cpu", size=24, center_crop=True)
    mapping = json.loads((root / "mapping_file.json").read_text())
    files = [root / "annotation_images" / e["image_path"] for e in mapping.values()]
    for name in ("mse", "ssim", "msssim"):
        res = yaml.safe_load((out / "metrics" / f"{name}.yaml").read_text())
        assert set(res) == {"name", "mean", "results"} and res["name"] == name
        assert [r["file"] for r in res["results"]] == stems[:3] and all(set(r) == {"value", "file"} for r in res["results"])
        vals = [r["value"] for r in res["results"]]
        assert math.isnan(vals[2]) and math.isnan(res["mean"])                     # the unreadable file raises: nan, and the mean of a list with a nan
        if name == "msssim":                                                       # 24 x 24 images: every sample raises
            assert all(math.isnan(v) for v in vals)
            continue
        for i in range(2):
            want = image_metrics(pre(out / "imgs" / f"{stems[i]}.png"), pre(files[i]), (-1, 1), (name,))[name].item()
            assert vals[i] == want and isinstance(vals[i], float)                  # (edit_image, source_image), both through the preprocessing
    assert "Image size should be larger than 160" in printed
    # a second run computes nothing and touches nothing
    before = {f.name: f.read_text() for f in (out / "metrics").iterdir()}
    compute_metrics.main(args)
    assert {f.name: f.read_text() for f in (out / "metrics").iterdir()} == before and len(before) == 4
    # default metric list: the built four; an unbuilt name is refused by name
    assert compute_metrics.parse_args(args).metric is None and sorted(before) == ["mse.yaml", "msssim.yaml", "psnr.yaml", "ssim.yaml"]
    with pytest.raises(NotImplementedError, match="pretrained CLIP"):
        compute_metrics.main(args + ["--metric", "lpips"])


def test_compute_metrics_mean_and_batches(tmp_path):
    import yaml
    import compute_metrics
    root, out, stems = _sweep(tmp_path)
    one, two = tmp_path / "b1", tmp_path / "b2"
    for dst, batch in ((one, "1"), (two, "32")):
        (dst / "imgs").mkdir(parents=True)
        for s in stems[:2]:
            (dst / "imgs" / f"{s}.png").write_bytes((out / "imgs" / f"{s}.png").read_bytes())
        compute_metrics.main(["--data_path", str(root), "--output", str(dst), "--device", "cpu", "--size", "24", "--batch", batch, "--metric", "mse", "ssim"])
    for name in ("mse", "ssim"):
        a, b = (yaml.safe_load((d / "metrics" / f"{name}.yaml").read_text()) for d in (one, two))
        assert a == b and len(a["results"]) == 2                                   # the batch size changes nothing
        assert a["mean"] == float(np.mean([r["value"] for r in a["results"]]))
