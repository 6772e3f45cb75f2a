"""The lpips and bglpips metrics end to end on the device: preprocess, AlexNet tower, five distance calls, against float64.

The model is the library's synthetic AlexNet-width weights and the images come from the seeds of tests/lpips_ref.CASES (tests/golden/lpips_ref.npz,
written by tests/golden/make_lpips_golden.py, holds their float64 scores, a subset of their tap values -- tests/test_lpips_ref.py checks that
lpips_ref reproduces both -- and the yardsticks):
  s64, s67   4 pairs at 64 x 64 and at 67 x 70 (the pool's floor drops a row, conv1 leaves columns unread); even pairs are a source and the source
             plus noise 0.1 (a reconstruction), odd pairs independent images
  m64, m67   the same pairs with a foreground rectangle per pair (bglpips)
  big        one pair at 512 x 512: the workload's 127 / 63 / 31 geometry and large grids, against its recorded float64 score
Taps: with e_F = max |F_gpu - F_64| and y_F = max |F_prec - F_64| of lpips_ref run by torch on the CPU with every operand and result rounded to that
dtype and float32 arithmetic between two rounding points (dino_ref.Prec; recorded in the fixture), the test requires e_F <= 4 y_F per tap.
Scores: r = max over the pairs of |s - s_64| / s_64 must be at most 4 y_S, the same quantity of that CPU run over all 16 pairs of the four small
cases, so that one lucky draw does not set it; every s_64 exceeds 1e-4 (tests/test_lpips_ref.py).  The factor 4 is the one of
tests/test_dino_gpu.py, for its reasons: y is one draw of a maximum of rounding noise, and the kernels round at other points than the emulation
(the order of the fp32 additions inside a convolution; the preprocess rounds once from float64).
Measured e_F / y_F and r / y_S on MI355X: DESIGN.md, note `lpips`."""
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import lpips_ref as lr

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / "golden"
DTYPES = [torch.float16, torch.bfloat16, torch.float32]
name_of = lambda dt: str(dt).split(".")[-1]


@pytest.fixture(scope="module")
def fx():
    """the state dict and, per small case, the images, masks, float64 taps and scores -- computed once, shared, not modified"""
    z = np.load(GOLDEN / "lpips_ref.npz")
    sd = lr.model_state_dict()
    out = {"z": z, "sd": sd}
    for case in lr.SMALL:
        x, b, mask = lr.case_inputs(case)
        s64, t64 = lr.score(sd, x, b, -1, 1, mask)
        assert (s64 - torch.from_numpy(z[f"score_{case}"])).abs().max() <= 1e-13            # the fixture's cases, as recorded
        out[case] = dict(x=x, b=b, mask=mask, s64=s64, t64=[t.flatten(2).transpose(1, 2) for t in t64])
    return out


@pytest.fixture(scope="module")
def models(fx):
    from metrics import LpipsModel
    return {dt: LpipsModel(fx["sd"], "cuda", compute_dtype=dt) for dt in DTYPES}


@pytest.mark.parametrize("dtype", DTYPES, ids=name_of)
@pytest.mark.parametrize("case", lr.SMALL)
def test_small_cases_taps_and_scores(fx, models, case, dtype):
    from metrics import lpips_distance
    from metrics.lpips import lpips_taps
    c, z, nm, model = fx[case], fx["z"], name_of(dtype), models[dtype]
    x, b = c["x"].cuda(), c["b"]
    mask = None if c["mask"] is None else c["mask"].cuda()
    taps = lpips_taps(x, model, mask=mask)
    ratios = []
    for l, (t, t64) in enumerate(zip(taps, c["t64"])):
        assert t.dtype == dtype and t.shape == t64.shape and t.is_cuda
        e_f, y_f = (t.double().cpu() - t64).abs().max().item(), float(z[f"y_F_{case}_{l}_{nm}"])
        ratios.append(e_f / y_f)
    got = lpips_distance(x[b:], x[:b], model, mask=mask)
    assert got.dtype == torch.float64 and got.shape == (b,)
    r, y_s = ((got.cpu() - c["s64"]).abs() / c["s64"]).max().item(), float(z[f"y_S_{nm}"])
    print(f"lpips-e2e {case} {nm}: e_F/y_F per tap {[round(v, 2) for v in ratios]}; score r {r:.3e} y_S {y_s:.3e} r/y_S {r / y_s:.2f}")
    assert max(ratios) <= 4, (case, nm, ratios)
    assert r <= 4 * y_s, (case, nm, r, y_s)


@pytest.mark.parametrize("dtype", DTYPES, ids=name_of)
def test_one_pair_at_512(fx, models, dtype):
    from metrics import lpips_distance
    x, b, _ = lr.case_inputs("big")
    s64, nm = float(fx["z"]["score_big"][0]), name_of(dtype)
    got = lpips_distance(x[b:].cuda(), x[:b].cuda(), models[dtype])
    assert [tuple(t.shape) for t in models[dtype].backend._buffers[(2, 512, 512, "cuda:0")][0]] == [(2, 127 * 127, 64), (2, 63 * 63, 192), (2, 961, 384),
                                                                                                     (2, 961, 256), (2, 961, 256)]
    r, y_s = abs(float(got[0]) - s64) / s64, float(fx["z"][f"y_S_{nm}"])
    print(f"lpips-e2e big {nm}: score {float(got[0]):.9f} s_64 {s64:.9f} r {r:.3e} y_S {y_s:.3e} r/y_S {r / y_s:.2f}")
    assert r <= 4 * y_s, (nm, r, y_s)


def test_scores_do_not_depend_on_the_batch_repeat_and_vanish_for_equal_images(fx, models):
    from metrics import lpips_distance
    c, model = fx["m67"], models[torch.float16]
    src, edit, mask = c["x"][:4].cuda(), c["x"][4:].cuda(), c["mask"].cuda()
    bits = lambda t: t.cpu().view(torch.int64)
    for mk in (None, mask):
        full, again = lpips_distance(edit, src, model, mask=mk), lpips_distance(edit, src, model, mask=mk)
        assert torch.equal(bits(full), bits(again))
        for i in range(4):
            alone = lpips_distance(edit[i:i + 1], src[i:i + 1], model, mask=None if mk is None else mk[i:i + 1])
            assert torch.equal(bits(alone), bits(full[i:i + 1])), i
        assert torch.equal(bits(lpips_distance(src, edit, model, mask=mk)), bits(full))            # the sides swapped
        assert float(lpips_distance(src, src, model, mask=mk).abs().max()) == 0.0
    one = lpips_distance(edit, src, model, mask=mask[0])                                             # an (H, W) mask serves every pair
    assert torch.equal(bits(one[:1]), bits(lpips_distance(edit, src, model, mask=mask)[:1])) and not torch.equal(bits(one[1:2]), bits(full[1:2]))


def test_classes_and_edit_metric_on_the_device(fx):
    from metrics import EditMetric, lpips_distance
    c = fx["m64"]
    x, mask = c["x"], c["mask"]
    m = EditMetric("lpips", device="cuda", lpips_weights="synthetic")
    bg = EditMetric("bglpips", device="cuda", lpips_weights=m.metric.model)
    assert repr(m) == "lpips" and repr(bg) == "bglpips" and m.metric.model.device == "cuda" and bg.metric.model.backend is m.metric.model.backend
    model = m.metric.model
    vals = [m.update(x[i:i + 1], x[4 + i:5 + i], "a cat", "a dog", "dog") for i in range(2)]
    want = [float(lpips_distance(x[4 + i:5 + i].cuda(), x[i:i + 1].cuda(), model)[0]) for i in range(2)]
    assert vals == want and all(v > 0 for v in vals)
    got = [bg.update(x[i:i + 1], x[4 + i:5 + i], "a cat", "a dog", "dog", mask[i]) for i in range(2)]
    want = [float(lpips_distance(x[4 + i:5 + i].cuda(), x[i:i + 1].cuda(), model, mask=mask[i:i + 1].cuda())[0]) for i in range(2)]
    assert got == want and got != vals
    assert bg.update(x[:1], x[4:5], "a cat", "a dog", "dog", None) is None and len(bg.metric.losses) == 2
    mean, info = bg.compute()
    assert mean == float(np.mean(got)) and info["all"] == got
    assert m.metric(x[:4], x[4:]).shape == (4, 1, 1, 1)
    with pytest.raises(ValueError, match="at least 31 x 31"):
        lpips_distance(torch.zeros(1, 3, 30, 40, device="cuda"), torch.zeros(1, 3, 30, 40, device="cuda"), model)
