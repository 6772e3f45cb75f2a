"""The dinovitstruct_v2 metric end to end on the device: patch-14 preprocess, DINOv2 tower with the fused LayerScale + LayerNorm step and the
interpolated position table, keys, fused self-similarity distance, against float64.

Models and images are drawn from the seeds of tests/dinov2_ref.CASES (tests/golden/dinov2_ref.npz, written by tests/golden/make_dinov2_golden.py,
holds their float64 scores and keys -- tests/test_dinov2_ref.py checks that dinov2_ref reproduces both -- and the yardsticks):
  case A   width 128, 3 layers, image 42, table 5 x 5 -> 3 x 3 (10 tokens); 8 pairs at S = 20 (upscale) and 8 pairs at S = 64
  case B   width 128, 2 layers, image 224, table 37 x 37 -> 16 x 16 (257 tokens: one past four 64-wide tiles); 2 pairs at S = 256
  syn      the library's synthetic weights at "tinyv2/14", on case A's S = 20 pairs
The conditions are those of tests/test_dino_gpu.py (its docstring has the reasoning): e_K = max |K_gpu - K_64| <= 4 y_K and
r = max over the pairs of |s_gpu - s_64| / s_64 <= 4 y_S, with y_K and y_S what dinov2_ref's tower gives on the CPU with every operand and
result rounded to that dtype and float32 arithmetic between two rounding points (the fixture records them; the maker asserts that every s_64
exceeds 1e-3).  y is one draw of a maximum of rounding noise and the kernels round at other points than the emulation, hence the factor 4.
Measured e_K / y_K and r / y_S on MI355X: DESIGN.md, note 4.9i."""
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import dinov2_ref as v2

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / "golden"
DTYPES = [torch.float16, torch.bfloat16, torch.float32]
name_of = lambda dt: str(dt).split(".")[-1]


@pytest.fixture(scope="module")
def fx():
    """per case: the state dict, the images, the float64 keys and scores -- computed once, shared, not modified"""
    z = np.load(GOLDEN / "dinov2_ref.npz")
    out = {"z": z}
    for case in v2.CASES:
        sd, image, x, b = v2.case_inputs(case)
        k64 = v2.image_keys(sd, x, -1, 1, image=image)
        s64 = v2.score(k64[:b], k64[b:])
        assert (s64 - torch.from_numpy(z[f"score_{case}"])).abs().max() <= 1e-12            # the fixture's cases, as recorded
        out[case] = dict(sd=sd, image=image, x=x, b=b, k64=k64, s64=s64)
    return out


def _run(fx, case, dtype, model):
    from metrics import dino_structure
    c, z, nm = fx[case], fx["z"], name_of(dtype)
    x, b = c["x"].cuda(), c["b"]
    keys = model.keys(x)
    assert keys.dtype == dtype and keys.shape == c["k64"].shape and keys.is_cuda
    e_k, y_k = (keys.double().cpu() - c["k64"]).abs().max().item(), float(z[f"y_K_{case}_{nm}"])
    got = dino_structure(x[b:], x[:b], model)
    assert got.dtype == torch.float64 and got.shape == (b,)
    r, y_s = ((got.cpu() - c["s64"]).abs() / c["s64"]).max().item(), float(z[f"y_S_{case}_{nm}"])
    print(f"dinov2-e2e {case} {nm}: e_K {e_k:.3e} y_K {y_k:.3e} e_K/y_K {e_k / y_k:.2f}; score r {r:.3e} y_S {y_s:.3e} r/y_S {r / y_s:.2f}")
    assert e_k <= 4 * y_k, (case, nm, e_k, y_k)
    assert r <= 4 * y_s, (case, nm, r, y_s)


@pytest.mark.parametrize("dtype", DTYPES, ids=name_of)
@pytest.mark.parametrize("case", ["a20", "a64"])
def test_fixture_model_case_a(fx, case, dtype):
    from metrics import Dinov2Model
    model = Dinov2Model(fx[case]["sd"], "cuda", compute_dtype=dtype, image=fx[case]["image"])
    assert (model.patch, model.image, model.width, model.table, len(model.backend.layers)) == (14, 42, 128, 5, 2)
    _run(fx, case, dtype, model)


@pytest.mark.parametrize("dtype", DTYPES, ids=name_of)
def test_fixture_model_case_b_at_257_tokens(fx, dtype):
    from metrics import Dinov2Model
    model = Dinov2Model(fx["b"]["sd"], "cuda", compute_dtype=dtype)
    assert (model.patch, model.image, model.table, model.backend.g2 + 1) == (14, 224, 37, 257)
    _run(fx, "b", dtype, model)


@pytest.mark.parametrize("dtype", DTYPES, ids=name_of)
def test_synthetic_weights(fx, dtype):
    from metrics import Dinov2Model
    _run(fx, "syn", dtype, Dinov2Model("synthetic", "cuda", "tinyv2/14", compute_dtype=dtype))


def test_the_other_table_form_is_another_model(fx):
    """interpolate_offset = 0 (transformers' form) against float64 with the same offset, and away from the offset-0.1 keys"""
    from metrics import Dinov2Model
    c = fx["b"]
    model = Dinov2Model(c["sd"], "cuda", interpolate_offset=0.0)
    keys = model.keys(c["x"][:1].cuda()).double().cpu()
    k0 = v2.image_keys(c["sd"], c["x"][:1], -1, 1, offset=0.0)
    assert (keys - k0).abs().max().item() <= 4 * float(fx["z"]["y_K_b_float16"])
    assert (keys - c["k64"][:1]).abs().max().item() > 0.05


def test_scores_do_not_depend_on_the_batch_and_repeat(fx):
    from metrics import Dinov2Model, dino_structure
    c = fx["a64"]
    model = Dinov2Model(c["sd"], "cuda", image=c["image"])
    src, edit = c["x"][:4].cuda(), c["x"][8:12].cuda()
    full, again = dino_structure(edit, src, model), dino_structure(edit, src, model)
    assert torch.equal(full.view(torch.int64), again.view(torch.int64))
    for i in range(4):
        assert torch.equal(dino_structure(edit[i:i + 1], src[i:i + 1], model).view(torch.int64), full[i:i + 1].view(torch.int64)), i


def test_edit_metric_on_the_device_equals_dino_structure(fx):
    from metrics import EditMetric, dino_structure
    x = fx["syn"]["x"]
    m = EditMetric("dinovitstruct_v2", device="cuda", dinov2_weights="synthetic", dinov2_model="tinyv2/14")
    assert repr(m) == "tinyv2/14" and m.metric.model.device == "cuda"
    vals = [m.update(x[i:i + 1], x[8 + i:9 + i], "a cat", "a dog", "dog") for i in range(2)]
    want = [float(dino_structure(x[i:i + 1].cuda(), x[8 + i:9 + i].cuda(), m.metric.model)[0]) for i in range(2)]       # (source, edit) as update passes them
    assert vals == want and all(v > 0 for v in vals)
    mean, info = m.compute()
    assert mean == float(np.mean(vals)) and info["all"] == vals
    with pytest.raises(ValueError, match="square"):
        m.metric.model.keys(torch.zeros(1, 3, 42, 56, device="cuda"))
