"""tests/regdiff_ref.py (the restatement of regularised DDIM inversion that the GPU tests compare the engine with) against fixtures recorded
from the reference implementation's own RegularizedDiffusionInversion (tests/golden/make_regdiff_golden.py --reference), its two forms
against each other, its shift table against the generator call sequence, and the condition on the kernel tests' input.  CPU only."""
import numpy as np
import pytest
import torch

from tests import regdiff_ref as rr
from tests.golden.make_regdiff_golden import E2E_L, E2E_S, REG_SIZES, REG_VARIANTS, reg_keep


def test_level_sizes():
    """the pyramids the issue lists, and the sizes around the stop rule (a level of 8 is not pooled, 9 is)"""
    assert rr.level_sizes(64) == [64, 32, 16, 8] and rr.level_sizes(96) == [96, 48, 24, 12, 6]
    assert rr.level_sizes(20) == [20, 10, 5] and rr.level_sizes(44) == [44, 22, 11, 5]
    assert rr.level_sizes(8) == [8] and rr.level_sizes(9) == [9, 4] and rr.level_sizes(16) == [16, 8] and rr.level_sizes(17) == [17, 8]
    assert max(len(rr.level_sizes(L)) for L in range(8, 97)) == 5


@pytest.mark.parametrize("L", [8, 16, 20, 24, 44, 64, 96])
def test_closed_form_equals_autograd(L):
    x = rr.multiscale_field(L, 1, seed=L)[0].double()
    sh = rr.shift_table(L)
    closed = rr.regularize_closed(x.numpy(), sh)
    auto = rr.regularize_autograd(x, sh, dtype=torch.float64).numpy()
    err = np.abs(closed - auto).max()
    print(f"L = {L}: closed form vs float64 autograd max-abs {err:.3e} on outputs up to {np.abs(auto).max():.2f}")
    assert err <= 1e-12
    assert np.abs(closed - x.numpy()).max() > 1e-2                          # (and the regulariser moves the input)


@pytest.mark.parametrize("tag", list(REG_VARIANTS))
@pytest.mark.parametrize("L", REG_SIZES)
def test_both_forms_vs_reference(golden, L, tag):
    g = golden("regdiff_reg")
    x = rr.multiscale_field(L, 1, seed=L)
    np.testing.assert_array_equal(x.numpy().ravel()[:4], g[f"probe/L{L}"])
    kw = {**rr.DEFAULTS, **REG_VARIANTS[tag]}
    sh = rr.shift_table(L, kw["num_reg_steps"], kw["num_ac_rolls"], kw["lambda_ac"])
    want = g[f"{tag}/L{L}"]
    closed = rr.regularize_closed(x[0].double().numpy(), sh, **kw).ravel()[reg_keep(L)]
    auto = rr.regularize_autograd(x[0], sh, dtype=torch.float64, **kw).numpy().ravel()[reg_keep(L)]
    assert want.dtype == np.float64 and want.shape == closed.shape
    # 1e-12 of the result's scale.  The scale is 1 wherever the iteration converges; with num_ac_rolls = 1 the autocorrelation step is five
    # times longer and at small sizes the iteration diverges (L = 8: values around 1e96) -- the reference's own behaviour, recorded as it is
    scale = max(1.0, np.abs(want).max())
    e_c, e_a = np.abs(closed - want).max() / scale, np.abs(auto - want).max() / scale
    print(f"L = {L} {tag}: vs the reference's float64 run (scale {scale:.1e}): closed form {e_c:.3e}, autograd restatement {e_a:.3e}")
    assert np.isfinite(want).all() and e_c <= 1e-12 and e_a <= 1e-12


def test_loop_vs_reference(golden):
    """RegDiffRef over the toy oracle UNet vs the reference's `invert` (fp32 there), at the bounds tests/test_edict_ref.py holds e2e_edict to"""
    from oracle.unet import build_unet
    from tests.edict_ref import torch_unet
    g, d = golden("e2e_regdiff"), golden("e2e_diffinv")
    ctx = d["ctx_src"]
    np.testing.assert_array_equal(np.concatenate([ctx.ravel()[:4], ctx.ravel()[-4:]]), g["ctx_probe"])
    assert int(g["S"]) == E2E_S and g["z0"].shape == (1, 4, E2E_L, E2E_L)
    toy = build_unet(0, block_out_channels=(32, 64, 128, 128))
    lat, eps = rr.RegDiffRef(torch_unet(toy), E2E_S).invert(g["z0"], ctx)
    np.testing.assert_allclose(lat[:, 0], g["inv_latents"], rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(eps[:, 0], g["noise_preds"], rtol=1e-4, atol=2e-5)
    off, _ = rr.RegDiffRef(torch_unet(toy), E2E_S, regularize=False).invert(g["z0"], ctx)
    assert np.abs(off[-1] - lat[-1]).max() > 1e-2                           # the regularisation is not a no-op on this trajectory


@pytest.mark.parametrize("L", [8, 20, 96])
def test_shift_table_is_the_generator_call_sequence(L):
    sizes = rr.level_sizes(L)
    table = rr.shift_table(L)
    assert table.shape == (25, 4, len(sizes)) and table.dtype == np.int32
    gen = torch.Generator().manual_seed(0)
    for a in range(25):                                                     # autocorrelation step, then channel, then level from fine to coarse
        for c in range(4):
            for k, s in enumerate(sizes):
                assert table[a, c, k] == torch.randint(0, s // 2, (), generator=gen).item()
    assert (table >= 0).all() and all((table[:, :, k] < s // 2).all() for k, s in enumerate(sizes))
    assert (table == 0).any()                                               # r = 0 occurs
    np.testing.assert_array_equal(table, rr.shift_table(L, generator=torch.Generator().manual_seed(0)))
    assert rr.shift_table(L, lambda_ac=0.0).shape == (0, 4, len(sizes))     # nothing is drawn
    assert rr.shift_table(L, num_reg_steps=2, num_ac_rolls=1).shape == (2, 4, len(sizes))


@pytest.mark.parametrize("L", rr.KERNEL_SIZES)
def test_every_level_matters_on_the_kernel_input(L):
    """the kernel tests mean something only if a kernel that loses one pyramid level, or reads one level's shift wrong, misses their bound by far:
    per image, dropping any one level or offsetting any one level's shift by one moves the float64 result by at least 100 x the bound"""
    case = rr.kernel_case(L)
    worst = np.inf
    for img in range(case["x"].shape[0]):
        x = case["x"][img].double().numpy()
        for k in range(len(rr.level_sizes(L))):
            for kw in (dict(drop_level=k), dict(bump_level=k)):
                moved = np.abs(rr.regularize_closed(x, case["shifts"], **case["params"], **kw) - case["ref"][img]).max()
                worst = min(worst, moved / case["bound"][img])
                assert moved >= 100 * case["bound"][img], (L, img, kw, moved, case["bound"][img])
    print(f"L = {L}: fp32 restatement within {case['dev32'].max():.3e} of float64; smallest (change of one level) / bound = {worst:.0f}")
