"""The float64 restatement of the image metrics (tests/metrics_ref.py) against the reference: its own float32 values of the seeded cases
(tests/golden/metrics_ref.npz, written by tests/golden/make_metrics_golden.py from the reference's classes) and the four floats it recorded for
its test pair of PNGs.

Bounds.  Seeded cases: the yardstick of the fixture, the largest |reference float32 - float64| per metric -- by construction; what this pins is
that the restatement in the tree is the one the fixture was made with.  PNG pair: mse and psnr relative 1e-6 (float32 sums of 786,432 terms);
msssim 6e-7 and ssim 2e-5 absolute, twice the gap between the float64 value and the recorded float32 one (0.77499505 against 0.77499479,
0.68140361 against 0.68139368: the cancellation in E[x^2] - mu^2 costs float32 the fifth decimal on a smooth photograph)."""
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import metrics_ref as mr

GOLDEN = Path(__file__).resolve().parent / "golden"
PNG_BOUNDS = {"mse": ("rel", 1e-6), "psnr": ("rel", 1e-6), "msssim": ("abs", 6e-7), "ssim": ("abs", 2e-5)}


def png_pair(device="cpu"):
    """(source, edit) of the reference's metric test, preprocessed as its compute_metrics does"""
    from modules.models import StablePreprocess
    pre = StablePreprocess(device, size=512, center_crop=True)
    return pre(GOLDEN / "gnochi_mirror_sq.png"), pre(GOLDEN / "gnochi_mirror_sq_edit_example.png")


def within(value, want, kind, bound):
    err = abs(value - want) / (abs(want) if kind == "rel" else 1.0)
    return err <= bound, err


@pytest.fixture(scope="module")
def fixture():
    return np.load(GOLDEN / "metrics_ref.npz")


def test_fixture_holds_every_case(fixture):
    assert list(fixture["cases"]) == [c[0] for c in mr.CASES]
    for name, h, w, seed in mr.CASES:
        assert fixture[f"{name}/shape"].tolist() == [h, w] and int(fixture[f"{name}/seed"]) == seed
        want = {"mse", "psnr", "ssim"} | ({"msssim"} if min(h, w) > 160 else set())
        assert {k.split("/")[1] for k in fixture.files if k.startswith(f"{name}/") and k.endswith("/ref32")} == want
    for n in mr.NAMES:
        assert 0 < float(fixture[f"yardstick/{n}"]) < 1e-5


@pytest.mark.parametrize("case", mr.CASES, ids=[c[0] for c in mr.CASES])
def test_restatement_within_yardstick_of_reference(fixture, case):
    name = case[0]
    got = mr.all_metrics(*mr.make_pair(*case))
    for n, v in got.items():
        yard, ref32 = float(fixture[f"yardstick/{n}"]), float(fixture[f"{name}/{n}/ref32"])
        print(f"{name} {n}: float64 {v!r} reference float32 {ref32!r} |diff| {abs(v - ref32):.3g} yardstick {yard:.3g}")
        assert abs(v - ref32) <= yard
        assert v == float(fixture[f"{name}/{n}/f64"])          # the restatement the fixture was made with


def test_restatement_meets_recorded_floats_on_png_pair(fixture):
    source, edit = png_pair()
    assert source.shape == (1, 3, 512, 512)
    got = mr.all_metrics(edit[0], source[0])
    for n, (kind, bound) in PNG_BOUNDS.items():
        ok, err = within(got[n], float(fixture[f"recorded/{n}"]), kind, bound)
        print(f"{n}: float64 {got[n]!r} recorded {float(fixture[f'recorded/{n}'])!r} {kind} error {err:.3g} bound {bound:g}")
        assert ok, (n, got[n], err)
    assert abs(mr.data_range(edit[0], source[0]) - 1.0) < 1e-12      # this pair spans the whole range: it does not test the range-from-data rule


def test_degenerate_pairs():
    pairs = mr.degenerate_pairs()
    same = mr.all_metrics(*pairs["identical"])
    assert same["mse"] == 0 and same["psnr"] == float("inf") and same["ssim"] == 1 and same["msssim"] == 1
    const = mr.all_metrics(*pairs["constants"])
    # x = 0.375, y = 0.75: the luminance term alone, 2 x y / (x^2 + y^2) = 0.8; in msssim it enters at the last level only, as 0.8^0.1333 = 0.9707,
    # and the zero padding of the odd sides puts an edge into the pooled constants
    assert abs(const["ssim"] - 0.8) < 1e-12 and 0.9 < const["msssim"] < 0.9707 and abs(const["mse"] - 0.375 ** 2) < 1e-15
    anti = mr.all_metrics(*pairs["anticorrelated"])
    assert anti["msssim"] == 0 and anti["ssim"] < 0
    assert all(np.isfinite(v) for d in (const, anti) for v in d.values())
    zero = torch.full((3, 11, 11), -1.0)
    assert mr.ssim(zero, zero) == 1                                   # 0 / 0: both images 0


def test_pooling_matches_torch():
    x = torch.rand(3, 21, 16, dtype=torch.float64)
    for h, w in ((21, 16), (20, 15), (21, 15)):
        got = mr.pool(x[:, :h, :w])
        want = torch.nn.functional.avg_pool2d(x[None, :, :h, :w], kernel_size=2, padding=[h % 2, w % 2])[0]
        assert got.shape == want.shape and torch.allclose(got, want, rtol=0, atol=1e-15)
