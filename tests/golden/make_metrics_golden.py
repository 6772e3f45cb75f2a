#!/usr/bin/env python3
"""Fixture generator for the image metrics: tests/golden/metrics_ref.npz.  CPU only.

    python tests/golden/make_metrics_golden.py --reference <checkout of the reference project>

RUNS THE REFERENCE'S OWN CODE: metrics/base.py, metrics/metrics.py (MSEMetric, PSNRMetric) and metrics/msssim.py (MSSSIM, ssim), loaded file by
file under a stub `metrics` package, because the reference's metrics/__init__.py imports lpips and CLIP.  They run in float32 on the seeded
pairs of tests/metrics_ref.py, one pair per call as the reference calls them.

[3P] The reference's SSIM class is torchmetrics.image.StructuralSimilarityIndexMeasure(), which is not installed where this runs.  Its float32
value is taken from the reference's own `metrics.msssim.ssim` (the same window, constants and unpadded filtering; reflect padding by 5 cropped
by 5 again is the unpadded region) given what torchmetrics' default data_range=None documents: the range of the normalised pair,
max(pred.max() - pred.min(), target.max() - target.min()).  The one anchor to the class itself is the float the reference recorded for its
test pair (RECORDED below, reference test/test_metrics.py:59-62).

Per case the file holds shape, seed, the reference's float32 value and the float64 restatement's (tests/metrics_ref.py); per metric the
YARDSTICK: the largest |reference float32 - float64 restatement| over the seeded cases, which is what float32 arithmetic costs the reference
itself and what the kernel's and the CPU path's bounds are made of.  Nothing under tests/ reads the reference at test time."""
import argparse
import importlib.util
import sys
import types
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(REPO))
from tests import metrics_ref as mr  # noqa: E402

RECORDED = {"ssim": 0.6813936829566956, "msssim": 0.7749947905540466, "mse": 0.011490068398416042, "psnr": 19.396774291992188}


def load_reference(ref: Path):
    pkg = types.ModuleType("metrics")
    pkg.__path__ = [str(ref / "metrics")]
    sys.modules["metrics"] = pkg
    mods = {}
    for name in ("base", "metrics", "msssim"):
        spec = importlib.util.spec_from_file_location(f"metrics.{name}", ref / "metrics" / f"{name}.py")
        mod = importlib.util.module_from_spec(spec)
        sys.modules[f"metrics.{name}"] = mod
        spec.loader.exec_module(mod)
        mods[name] = mod
    return mods


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    a = ap.parse_args()
    mods = load_reference(Path(a.reference))
    crit = {"mse": mods["metrics"].MSEMetric(input_range=(-1, 1), device="cpu"), "psnr": mods["metrics"].PSNRMetric(input_range=(-1, 1), device="cpu"),
            "msssim": mods["msssim"].MSSSIM(input_range=(-1, 1), device="cpu")}
    ref_ssim = mods["msssim"].ssim
    out, yard = {}, {n: 0.0 for n in mr.NAMES}
    names = []
    with torch.no_grad():
        for name, h, w, seed in mr.CASES:
            pred, target = mr.make_pair(name, h, w, seed)
            p, t = pred[None], target[None]
            ref32 = {"mse": crit["mse"](p, t).item(), "psnr": crit["psnr"](p, t).item()}
            x, y = (p + 1) / 2, (t + 1) / 2                                       # BaseMetric._normalize
            ref32["ssim"] = ref_ssim(x, y, data_range=torch.max(x.max() - x.min(), y.max() - y.min())).item()
            if min(h, w) > 160:
                ref32["msssim"] = crit["msssim"](p, t).item()
            f64 = mr.all_metrics(pred, target)
            names.append(name)
            out[f"{name}/shape"] = np.array([h, w], dtype=np.int64)
            out[f"{name}/seed"] = np.array(seed, dtype=np.int64)
            for n, v in ref32.items():
                out[f"{name}/{n}/ref32"] = np.array(v, dtype=np.float32)
                out[f"{name}/{n}/f64"] = np.array(f64[n], dtype=np.float64)
                yard[n] = max(yard[n], abs(float(np.float32(v)) - f64[n]))
                print(f"{name:14s} {n:7s} reference fp32 {v:.9g}  float64 {f64[n]:.12g}  |diff| {abs(v - f64[n]):.3g}")
    for n in mr.NAMES:
        out[f"yardstick/{n}"] = np.array(yard[n], dtype=np.float64)
        out[f"recorded/{n}"] = np.array(RECORDED[n], dtype=np.float64)
        print(f"yardstick {n}: {yard[n]:.3g}")
    out["cases"] = np.array(names)
    np.savez(REPO / "tests" / "golden" / "metrics_ref.npz", **out)


if __name__ == "__main__":
    main()
