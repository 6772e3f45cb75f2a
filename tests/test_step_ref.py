"""The float64 restatement of the fused backward step (tests/step_ref.py), the reference of the kernel tests in tests/test_small_kernels_gpu.py,
against the goldens recorded from the reference implementation: the reference is checked independently of the code under test.  No GPU."""
import numpy as np
import pytest
import torch

from tests import step_ref

ETA = ["lin_t980", "lin_t0", "paper_t600", "paper_t620", "paper_t980", "paper_t980_nomask"]
MODES = ["gt_thres", "fwd_t", "soft", "soft_pow", "thres_pow"]
DIRINV = ["tdir", "tdir_masked", "tdir_soft", "tdir_gt", "tdir_gt_eta_fwd"]


@pytest.mark.parametrize("name", ETA + MODES + DIRINV)
def test_eta_backward_step_restatement_reproduces_the_goldens(golden, name):
    """the cases and tolerances tests/test_kernels_gpu.py holds the kernel to"""
    from tests.golden import recipes
    which, kw = step_ref.golden_case(name)
    g = golden(which)
    inp = recipes.eta_case_inputs(name)
    assert [recipes.crc(inp[k]) for k in ("latent", "unet_out", "src_prev", "mask_map", "noise")] == list(g[f"{name}/crc"])
    out_x, _, best, losses = step_ref.eta_backward_step_ref(**kw)
    np.testing.assert_allclose(out_x.numpy(), g[f"{name}/new"], rtol=1e-4, atol=5e-5)
    if f"{name}/best" in g.files:
        assert int(best[0]) == int(g[f"{name}/best"])
    if f"{name}/losses" in g.files and np.isfinite(g[f"{name}/losses"]).all():
        np.testing.assert_allclose(losses[0].numpy(), g[f"{name}/losses"], rtol=2e-4)


@pytest.mark.parametrize("poison,expect", [({7: 3}, 3), ({6: None}, 6), ({8: None, 5: None}, 5)], ids=["tie", "nan_above_winner", "two_nans"])
def test_restatement_argmin_rule(poison, expect):
    """first NaN wins, else the first minimum (torch.argmin, which the reference uses at eta_inversion.py:330-375): candidate 3 is planted; a copy of it at 7
    loses the tie, a candidate with one NaN element wins over it, and of two such the lower index wins"""
    from oracle import schedule as sch
    ac, g = sch.alphas_cumprod(), torch.Generator().manual_seed(1)
    x, eps_all, noise = torch.randn(2, 4, 6, 6, generator=g), torch.randn(4, 4, 6, 6, generator=g), torch.randn(10, 4, 6, 6, generator=g)
    eps_s = eps_all[0].double() + step_ref.G * (eps_all[2].double() - eps_all[0].double())
    x_prev = (sch.ddim_eta_step(x[0].double(), eps_s, ac, 500, 50, 0.4) + 0.4 * sch.variance(ac, 500, 50) ** 0.5 * noise[3].double())[None]
    for j, src in poison.items():
        if src is None:
            noise[j, 1, 2, 3] = float("nan")
        else:
            noise[j] = noise[src]
    _, _, best, losses = step_ref.eta_backward_step_ref(x, eps_all, step_ref.G, x_prev, noise, 0.4, None, 0.2, 0, ac, 500, 50)
    assert int(best[0]) == expect
    assert torch.isnan(losses[0]).nonzero().flatten().tolist() == sorted(j for j, src in poison.items() if src is None)
