"""etainv_image_metrics (csrc/metrics.hip) through `metrics.image_metrics` on the device, against the float64 restatement (tests/metrics_ref.py;
its values of the seeded cases are in tests/golden/metrics_ref.npz, pinned to the restatement by tests/test_metrics_ref.py).

Bounds.  Seeded cases, per metric: |kernel - float64| <= 2 x the fixture's yardstick, the largest |reference float32 - float64| over the cases --
the kernel may not be less accurate than twice the reference's own float32 run (the factor: a different summation order).  Yardsticks:
mse 4.74e-10, psnr 1.74e-6, ssim 9.96e-8, msssim 1.67e-6.  Degenerate pairs: 1, 1, 0 and inf exactly where the issue states them; their other
values against float64 within the same bound plus half an ulp of the float32 result (the output is float32: an anti-correlated pair's mse of
0.33 cannot be nearer than 1.5e-8).  PNG pair against the floats the reference recorded: mse, psnr relative 1e-6, msssim 6e-7, ssim 2e-5
absolute (tests/test_metrics_ref.py).  Measured on MI355X: DESIGN.md, "Image metrics"."""
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import metrics_ref as mr

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / "golden"
PNG_BOUNDS = {"mse": ("rel", 1e-6), "psnr": ("rel", 1e-6), "msssim": ("abs", 6e-7), "ssim": ("abs", 2e-5)}


@pytest.fixture(scope="module")
def fixture():
    return np.load(GOLDEN / "metrics_ref.npz")


def names_for(h, w):
    return ("mse", "psnr", "ssim") + (("msssim",) if min(h, w) > 160 else ())


def run(pred, target, which=None, input_range=(-1, 1)):
    """pairs (B, 3, H, W) on the CPU -> {name: float32 numpy [B]} from the device"""
    from metrics import image_metrics
    which = which or names_for(*pred.shape[2:])
    out = image_metrics(pred.cuda(), target.cuda(), input_range, which)
    assert list(out) == list(which) and all(v.is_cuda and v.dtype == torch.float32 and v.shape == (pred.shape[0],) for v in out.values())
    return {n: v.cpu().numpy() for n, v in out.items()}


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def half_ulp32(v):
    return float(np.spacing(np.float32(abs(v)))) / 2


@pytest.fixture(scope="module")
def mixed():
    """B = 3 at one shape: a seeded pair, the two constants, the anti-correlated pair; with their float64 values"""
    deg = mr.degenerate_pairs()
    pairs = [mr.make_pair("161x176", 161, 176, 202), deg["constants"], deg["anticorrelated"]]
    want = [mr.all_metrics(p, t) for p, t in pairs]
    return torch.stack([p for p, _ in pairs]), torch.stack([t for _, t in pairs]), want


@pytest.mark.parametrize("case", mr.CASES, ids=[c[0] for c in mr.CASES])
def test_accuracy_seeded(fixture, case):
    name, h, w, _ = case
    pred, target = mr.make_pair(*case)
    got = run(pred[None], target[None])
    for n, v in got.items():
        want, bound = float(fixture[f"{name}/{n}/f64"]), 2 * float(fixture[f"yardstick/{n}"])
        print(f"{name} {n}: kernel {float(v[0])!r} float64 {want!r} |error| {abs(float(v[0]) - want):.3g} bound {bound:.3g}")
        assert abs(float(v[0]) - want) <= bound, (name, n)


def test_degenerate_pairs(fixture, mixed):
    deg = mr.degenerate_pairs()
    same = run(deg["identical"][0][None], deg["identical"][1][None])
    assert same["ssim"][0] == 1 and same["msssim"][0] == 1 and same["mse"][0] == 0 and same["psnr"][0] == np.inf
    pred, target, want = mixed
    got = run(pred, target)
    assert not any(np.isnan(v).any() for v in got.values())
    assert got["msssim"][2] == 0 and got["ssim"][2] < 0                  # anti-correlated: every fine level's cs is clamped at 0
    for i in (1, 2):
        for n, v in got.items():
            bound = 2 * float(fixture[f"yardstick/{n}"]) + half_ulp32(want[i][n])
            print(f"pair {i} {n}: kernel {float(v[i])!r} float64 {want[i][n]!r} |error| {abs(float(v[i]) - want[i][n]):.3g} bound {bound:.3g}")
            assert abs(float(v[i]) - want[i][n]) <= bound, (i, n)
    zero = torch.full((1, 3, 11, 11), -1.0)                              # both images 0 after normalisation: 0 / 0 is 1
    assert run(zero, zero, ("ssim",))["ssim"][0] == 1


def test_png_pair_through_edit_metric(fixture):
    from metrics import EditMetric
    from modules.models import StablePreprocess
    pre = StablePreprocess("cuda", size=512, center_crop=True)
    source, edit = pre(GOLDEN / "gnochi_mirror_sq.png"), pre(GOLDEN / "gnochi_mirror_sq_edit_example.png")
    for n, (kind, bound) in PNG_BOUNDS.items():
        m = EditMetric(n, input_range=(-1, 1), device="cuda")
        v = m.update(source_image=source, edit_image=edit, source_prompt="a cat sitting next to a mirror",
                     target_prompt="a tiger sitting next to a mirror", edit_word="cat")
        want = float(fixture[f"recorded/{n}"])
        err = abs(v - want) / (abs(want) if kind == "rel" else 1.0)
        print(f"{n}: kernel {v!r} recorded {want!r} {kind} error {err:.3g} bound {bound:g}")
        assert err <= bound, n
        assert m.compute() == (v, {"value": v, "all": [v]})


def test_range_comes_from_the_data(fixture):
    case = next(c for c in mr.CASES if c[0] == "64x64_narrow")
    pred, target = mr.make_pair(*case)
    got = float(run(pred[None], target[None], ("ssim",))["ssim"][0])
    bound = 2 * float(fixture["yardstick/ssim"])
    from_data, unit = mr.ssim(pred, target), mr.ssim(pred, target, data_range_override=1.0)
    assert 0.24 < mr.data_range(pred, target) < 0.26
    print(f"ssim: kernel {got!r} float64 with the range from the data {from_data!r}, with range 1 {unit!r}")
    assert abs(got - from_data) <= bound and abs(got - unit) > 10 * bound


def test_deterministic_and_batch_independent(mixed):
    pred, target, _ = mixed
    full = run(pred, target)
    again = run(pred, target)
    assert all(np.array_equal(bits(full[n]), bits(again[n])) for n in full)
    for i in range(3):
        one = run(pred[i:i + 1], target[i:i + 1])
        assert all(bits(one[n])[0] == bits(full[n])[i] for n in full), i
    for subset in (("ssim",), ("msssim",), ("mse",), ("psnr", "msssim"), ("ssim", "msssim"), ("mse", "ssim")):
        part = run(pred, target, subset)
        assert all(np.array_equal(bits(part[n]), bits(full[n])) for n in subset), subset


def test_raw_call_fills_unselected_slots_with_nan(mixed):
    from etainv import _capi
    pred, target = mixed[0].cuda(), mixed[1].cuda()
    lib = _capi.load()
    nbytes = lib.etainv_image_metrics_workspace_bytes(3, 161, 176, 5)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device="cuda")
    out = torch.full((3, 4), 7.0, device="cuda")
    _capi.check(lib.etainv_image_metrics(_capi.ptr(pred), _capi.ptr(target), 3, 161, 176, -1.0, 1.0, 5, _capi.ptr(out), _capi.ptr(ws), nbytes, _capi.stream_ptr()))
    o = out.cpu().numpy()
    assert np.isnan(o[:, [1, 3]]).all() and not np.isnan(o[:, [0, 2]]).any()
    full = run(mixed[0], mixed[1])
    assert np.array_equal(bits(o[:, 0]), bits(full["mse"])) and np.array_equal(bits(o[:, 2]), bits(full["ssim"]))


def test_input_range_and_conversions(mixed):
    pred, target, _ = mixed
    full = run(pred, target)
    # the same pairs as values in (0, 255): the normalisation happens inside the kernels (the float32 rescaling here moves a pixel by 2^-24 relative)
    scaled = run((pred + 1) * 127.5, (target + 1) * 127.5, input_range=(0, 255))
    assert all(np.allclose(scaled[n], full[n], rtol=2e-6, atol=2e-7) for n in full)
    from metrics import image_metrics
    wide = image_metrics(pred.double().cuda().permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2), target.cuda().half().float(), which=("mse",))
    assert wide["mse"].dtype == torch.float32 and bool(torch.isfinite(wide["mse"]).all())


def test_non_default_stream_sees_its_producer(mixed):
    from metrics import image_metrics
    pred, target, _ = mixed
    full = run(pred, target)
    src_p, src_t = pred.cuda(), target.cuda()
    buf_p, buf_t = torch.zeros_like(src_p), torch.zeros_like(src_t)
    work = torch.randn(2048, 2048, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for _ in range(8):                                               # keeps the stream busy in front of the producer
            work = work @ work * 1e-3
        buf_p.copy_(src_p)                                               # the producer, on the side stream
        buf_t.copy_(src_t)
        out = image_metrics(buf_p, buf_t)
    side.synchronize()
    assert all(np.array_equal(bits(out[n].cpu().numpy()), bits(full[n])) for n in full)
