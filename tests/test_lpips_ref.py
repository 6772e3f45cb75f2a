"""CPU-only checks of tests/lpips_ref.py, the float64 reference side of the lpips / bglpips tests: pinned to an nn.Sequential laid out at
torchvision's `features` indices and run by F.conv2d / F.max_pool2d, to the recorded fixture, and to the properties of LPIPS's definition that a
restatement can get wrong (the constants, where the epsilon sits, where the mask is applied, the tap sizes)."""
from pathlib import Path

import numpy as np
import pytest
import torch
from torch import nn

from tests import lpips_ref as lr

GOLDEN = Path(__file__).resolve().parent / "golden"


@pytest.fixture(scope="module")
def sd():
    return lr.model_state_dict()


def _features(sd):
    """torchvision's AlexNet `features`, index by index, in float64"""
    f = nn.Sequential(nn.Conv2d(3, 64, 11, 4, 2), nn.ReLU(), nn.MaxPool2d(3, 2), nn.Conv2d(64, 192, 5, padding=2), nn.ReLU(), nn.MaxPool2d(3, 2),
                      nn.Conv2d(192, 384, 3, padding=1), nn.ReLU(), nn.Conv2d(384, 256, 3, padding=1), nn.ReLU(), nn.Conv2d(256, 256, 3, padding=1),
                      nn.ReLU(), nn.MaxPool2d(3, 2))
    f.load_state_dict({k[len("features."):]: v for k, v in sd.items() if k.startswith("features.")}, strict=True)
    return f.double().eval()


def _lpips_torch(sd, x0, x1, lo, hi, mask=None):
    """LPIPS as the lpips package's forward states it, on nn modules: scores [B] and the five taps of x0"""
    shift, scale = torch.tensor(lr.SHIFT, dtype=torch.float64).view(1, 3, 1, 1), torch.tensor(lr.SCALE, dtype=torch.float64).view(1, 3, 1, 1)
    feats, taps = _features(sd), ([], [])
    for side, x in enumerate((x0, x1)):
        v = (x.double() - lo) / (hi - lo) * 2 - 1
        if mask is not None:
            v = v * (1 - mask.double())[:, None]
        h = (v - shift) / scale
        for i, layer in enumerate(feats):
            h = layer(h)
            if i in (1, 4, 7, 9, 11):
                taps[side].append(h)
    total = 0
    for l, (f0, f1) in enumerate(zip(*taps)):
        n0 = f0 / (torch.sqrt(torch.sum(f0 ** 2, dim=1, keepdim=True)) + 1e-10)
        n1 = f1 / (torch.sqrt(torch.sum(f1 ** 2, dim=1, keepdim=True)) + 1e-10)
        total = total + nn.functional.conv2d((n0 - n1) ** 2, sd[f"lin{l}.model.1.weight"].double()).mean([2, 3])
    return total.reshape(-1), taps[0]


@pytest.mark.parametrize("case", ["s64", "s67", "m64", "m67"])
def test_reference_equals_torch_modules_and_the_fixture(sd, case):
    z = np.load(GOLDEN / "lpips_ref.npz")
    x, b, mask = lr.case_inputs(case)
    with torch.no_grad():
        s64, taps = lr.score(sd, x, b, -1, 1, mask)
        want, want_taps = _lpips_torch(sd, x[:b], x[b:], -1, 1, mask)
    assert s64.dtype == torch.float64 and s64.min() > 1e-4
    assert ((s64 - want).abs() / want).max() <= 1e-12
    for l, (t, w) in enumerate(zip(taps, want_taps)):
        assert t.shape[1:] == w.shape[1:] and (t[:b] - w).abs().max() <= 1e-12 * max(1.0, float(w.abs().max())), l
        assert np.abs(t.flatten()[::lr.TAP_STRIDE].numpy() - z[f"tap{l}_{case}"]).max() <= 1e-11, l
    assert np.abs(s64.numpy() - z[f"score_{case}"]).max() <= 1e-13
    # odd pairs are independent images, even pairs reconstructions: an order of magnitude apart
    assert s64[1::2].min() > 5 * s64[0::2].max()


def test_fixture_is_complete_and_well_conditioned():
    z = np.load(GOLDEN / "lpips_ref.npz")
    for case in lr.CASES:
        assert z[f"score_{case}"].shape == (lr.CASES[case]["pairs"],) and z[f"score_{case}"].min() > 1e-4, case
    for name, lo, hi in (("float16", 1e-5, 1e-3), ("bfloat16", 1e-4, 1e-2), ("float32", 1e-9, 1e-6)):
        assert lo < float(z[f"y_S_{name}"]) < hi, name
        for case in lr.SMALL:
            for l in range(5):
                assert 0 < float(z[f"y_F_{case}_{l}_{name}"]) < 0.1, (case, l, name)
    assert (GOLDEN / "lpips_ref.npz").stat().st_size < 512 * 1024


def test_big_case_score_is_the_recorded_one(sd):
    z = np.load(GOLDEN / "lpips_ref.npz")
    x, b, _ = lr.case_inputs("big")
    s64, taps = lr.score(sd, x, b, -1, 1)
    assert [tuple(t.shape[2:]) for t in taps] == [(127, 127), (63, 63), (31, 31), (31, 31), (31, 31)]
    assert abs(float(s64[0]) - float(z["score_big"][0])) <= 1e-13


def test_constants_and_tap_sizes():
    assert lr.SHIFT == (-.030, -.088, -.188) and lr.SCALE == (.458, .448, .450) and lr.EPS == 1e-10
    assert lr.CONVS == (0, 3, 6, 8, 10) and lr.KERNELS == ((11, 4, 2), (5, 1, 2), (3, 1, 1), (3, 1, 1), (3, 1, 1))
    assert lr.tap_sizes(512, 512) == [(127, 127), (63, 63), (31, 31), (31, 31), (31, 31)]
    assert lr.tap_sizes(64, 64) == [(15, 15), (7, 7), (3, 3), (3, 3), (3, 3)]
    assert lr.tap_sizes(31, 31) == [(7, 7), (3, 3), (1, 1), (1, 1), (1, 1)]
    assert lr.tap_sizes(67, 70) == [(16, 16), (7, 7), (3, 3), (3, 3), (3, 3)]
    assert lr.tap_sizes(35, 38)[0] == (8, 8) and lr.tap_sizes(35, 39)[0] == (8, 9)            # 38 + 4 - 11 = 31: three trailing columns unread
    assert lr.pool_size(lr.out_size(30, 11, 4, 2)) == 2 and lr.pool_size(2) == 0          # 30 leaves no pixel at tap 3


def test_conv_and_pool_against_torch_at_the_edges():
    g = torch.Generator().manual_seed(5)
    for (cin, cout, k, stride, pad), (h, w) in [((3, 8, 11, 4, 2), (35, 38)), ((3, 8, 11, 4, 2), (31, 31)), ((8, 16, 5, 1, 2), (3, 7)), ((8, 16, 3, 1, 1), (1, 1)),
                                                ((8, 16, 3, 1, 1), (3, 2))]:
        x, wt, b = (torch.randn(s, generator=g, dtype=torch.float64) for s in ((2, cin, h, w), (cout, cin, k, k), (cout,)))
        assert (lr.conv2d(x, wt, b, stride, pad) - nn.functional.conv2d(x, wt, b, stride=stride, padding=pad)).abs().max() < 1e-12
    for h, w in [(15, 15), (16, 16), (7, 3), (3, 3), (16, 7)]:
        x = torch.randn(2, 5, h, w, generator=g, dtype=torch.float64) - 3.0                # mostly negative: a maximum that starts from 0 fails
        assert torch.equal(lr.maxpool3s2(x), nn.functional.max_pool2d(x, 3, 2))
    assert lr.maxpool3s2(torch.zeros(1, 1, 16, 15)).shape[-2:] == (7, 7)


def test_epsilon_is_added_to_the_norm():
    f0, f1, w = torch.zeros(1, 4, 1, 2, dtype=torch.float64), torch.zeros(1, 4, 1, 2, dtype=torch.float64), torch.tensor([0.5, 0.25, 1.0, 2.0])
    f1[0, :, 0, 0] = torch.tensor([3.0, 0.0, 4.0, 0.0])              # pixel 0: a zero vector against (3, 0, 4, 0); pixel 1: zero against zero
    got = float(lr.tap_distance(f0, f1, w)[0])
    assert got == pytest.approx((0.5 * 0.36 + 1.0 * 0.64) / 2, rel=1e-10) and np.isfinite(got)
    tiny = torch.full((1, 4, 1, 1), 1e-10, dtype=torch.float64)      # |f| = 2e-10: f / (|f| + 1e-10) = 1/3 per channel, a clamp would give 1/2
    assert float(lr.tap_distance(tiny, torch.zeros_like(tiny), torch.ones(4))[0]) == pytest.approx(4 / 9, rel=1e-9)


def test_mask_is_applied_between_the_range_map_and_the_scaling_layer():
    x = torch.full((2, 3, 2, 2), 0.25)
    mask = torch.tensor([[[1.0, 0.0], [0.5, 0.0]]])
    v = lr.preprocess(x, 0, 1, mask)
    for c in range(3):
        assert float(v[0, c, 0, 0]) == pytest.approx((0.0 - lr.SHIFT[c]) / lr.SCALE[c], rel=1e-12)          # foreground -> 0, not -1
        assert float(v[1, c, 0, 1]) == pytest.approx((-0.5 - lr.SHIFT[c]) / lr.SCALE[c], rel=1e-12)
        assert float(v[0, c, 1, 0]) == pytest.approx((-0.25 - lr.SHIFT[c]) / lr.SCALE[c], rel=1e-12)        # a fractional mask scales
    two = lr.preprocess(torch.full((4, 3, 2, 2), 0.5), -1, 1, torch.stack([mask[0], 1 - mask[0]]))
    assert torch.equal(two[0], two[2]) and torch.equal(two[1], two[3]) and not torch.equal(two[0], two[1])   # image i uses mask i % n_mask
    assert torch.equal(lr.preprocess(x * 255, 0, 255), lr.preprocess(x, 0, 1))


def test_zero_for_identical_images_and_symmetry(sd):
    x, b, mask = lr.case_inputs("m64")
    same, _ = lr.score(sd, torch.cat([x[:b], x[:b]]), b, -1, 1, mask)
    assert float(same.abs().max()) == 0.0
    fwd, _ = lr.score(sd, x, b, -1, 1, mask)
    rev, _ = lr.score(sd, torch.cat([x[b:], x[:b]]), b, -1, 1, mask)
    assert torch.equal(fwd, rev)
    # inside the foreground an edit changes nothing
    y = x.clone()
    y[b:] = torch.where(mask[:, None] > 0, -y[b:], y[b:])
    assert torch.equal(lr.score(sd, y, b, -1, 1, mask)[0], fwd)
