"""CPU-only checks of the `regdiffinv` inverter's host side: the C ABI's refusals (every one made before anything touches the device), the
native shift-table builder against the restatement's, the registry and constructor signature, and construction on a fake model."""
import inspect
import types

import numpy as np
import pytest
import torch

from tests import regdiff_ref as rr


class _Engine:
    L = 16
    lib = None


def _call(lib, **over):
    """etainv_noise_regularize with plausible arguments (non-null stand-in pointers: refused calls never dereference), overridden by name"""
    p1, p2, p3, p4 = 4096, 8192, 12288, 16384
    a = dict(eps_u=None, eps_c=p1, g=1.5, eps_out=p2, x=None, a_from=0.9, a_to=0.8, x_out=None, n_img=1, l=16, shifts=p3, num_reg_steps=5,
             num_ac_rolls=5, lambda_ac=20.0, lambda_kl=20.0)
    a.update(over)
    return lib.etainv_noise_regularize(a["eps_u"], a["eps_c"], a["g"], a["eps_out"], a["x"], a["a_from"], a["a_to"], a["x_out"], a["n_img"], a["l"],
                                       a["shifts"], a["num_reg_steps"], a["num_ac_rolls"], a["lambda_ac"], a["lambda_kl"], None)


def test_capi_refusals():
    from etainv import _capi
    lib = _capi.load()
    err = lambda: lib.etainv_last_error().decode()
    nan, inf = float("nan"), float("inf")
    refused = [
        (dict(eps_c=None), "null pointer"),
        (dict(eps_out=None), "null pointer"),
        (dict(shifts=None), "shifts_dev"),
        (dict(x=4096), "x_out"),
        (dict(l=7), "[8, 96]"),
        (dict(l=97), "[8, 96]"),
        (dict(l=0), "[8, 96]"),
        (dict(n_img=-1), "negative"),
        (dict(num_reg_steps=-1), "negative"),
        (dict(num_ac_rolls=-2), "negative"),
        (dict(eps_u=4096, g=nan), "g must be finite"),
        (dict(eps_u=4096, g=inf), "g must be finite"),
        (dict(lambda_ac=nan), "finite"),
        (dict(lambda_kl=-inf), "finite"),
        (dict(a_from=nan), "finite"),
        (dict(a_to=inf), "finite"),
        (dict(x=4096, x_out=8192, a_from=0.0), "(0,1]"),
        (dict(x=4096, x_out=8192, a_to=1.5), "(0,1]"),
        (dict(num_ac_rolls=0), "num_ac_rolls"),
    ]
    for over, fragment in refused:
        assert _call(lib, **over) != 0, over
        assert fragment in err() and "etainv_noise_regularize" in err(), (over, err())
    with pytest.raises(_capi.EtainvError, match="x_out"):
        _capi.check(_call(lib, x=4096))
    # n_img == 0: nothing to do, whatever else is asked for; a non-finite g without eps_u is ignored; no shift table is needed when no
    # autocorrelation step runs
    assert _call(lib, n_img=0) == 0
    assert _call(lib, n_img=0, g=nan) == 0
    assert _call(lib, n_img=0, shifts=None, lambda_ac=0.0) == 0
    assert _call(lib, n_img=0, shifts=None, num_reg_steps=0) == 0
    assert _call(lib, n_img=0, shifts=None, lambda_ac=0.0, num_ac_rolls=0) == 0
    assert _call(lib, n_img=0, l=8) == 0 and _call(lib, n_img=0, l=96) == 0


@pytest.mark.parametrize("L", [8, 16, 20, 44, 64, 96])
def test_native_shift_table_matches_restatement(L):
    from etainv.pipeline import regdiff_level_sizes, regdiff_shift_table
    assert regdiff_level_sizes(L) == rr.level_sizes(L)
    np.testing.assert_array_equal(regdiff_shift_table(L), rr.shift_table(L))
    np.testing.assert_array_equal(regdiff_shift_table(L, 2, 3, generator=torch.Generator().manual_seed(5)),
                                  rr.shift_table(L, 2, 3, generator=torch.Generator().manual_seed(5)))
    assert regdiff_shift_table(L, lambda_ac=0.0).shape == (0, 4, len(rr.level_sizes(L)))


def test_registry_and_signature():
    import modules
    from modules.inversion.regularized_diffusion_inversion import RegularizedDiffusionInversion
    assert "regdiffinv" in modules.get_inversion_methods()
    assert modules._inverters["regdiffinv"] is RegularizedDiffusionInversion and issubclass(RegularizedDiffusionInversion, modules.DiffusionInversion)
    sig = inspect.signature(RegularizedDiffusionInversion.__init__).parameters
    assert list(sig)[1:] == ["model", "scheduler", "num_inference_steps", "guidance_scale_bwd", "guidance_scale_fwd", "verbose", "lambda_ac",
                             "lambda_kl", "num_reg_steps", "num_ac_rolls"]
    assert [sig[n].default for n in ("lambda_ac", "lambda_kl", "num_reg_steps", "num_ac_rolls")] == [20.0, 20.0, 5, 5]
    for name in ("auto_corr_loss", "kl_divergence", "regularize_noise_pred", "predict_step_forward", "diffusion_forward"):
        assert name in vars(RegularizedDiffusionInversion), name
    with pytest.raises(NotImplementedError) as e:                          # the message of what is still missing names what exists
        modules.load_inverter("npi", model=None)
    assert "regdiffinv" in str(e.value)
    from etainv import _capi
    assert len(_capi.SIGNATURES["etainv_noise_regularize"]) == 16 and hasattr(_capi.load(), "etainv_noise_regularize")


def _fake_model():
    from modules.schedulers import DDIMScheduler
    sched = DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", clip_sample=False, set_alpha_to_one=False)
    return types.SimpleNamespace(unet=None, device="cpu", scheduler=sched, engine=_Engine())


def test_plugin_construction_and_losses():
    """what the constructor builds without touching the device; the two loss helpers against the restatement's"""
    import modules
    from etainv.pipeline import NoiseRegularizer
    from modules.editing.controller import ControllerBase, ControllerEmpty
    inv = modules.load_inverter("regdiffinv", model=_fake_model(), num_inference_steps=4)
    assert (inv.lambda_ac, inv.lambda_kl, inv.num_reg_steps, inv.num_ac_rolls) == (20.0, 20.0, 5, 5)
    assert isinstance(inv._reg, NoiseRegularizer) and inv._loop.regularizer is inv._reg and inv._reg.L == 16
    assert inv._loop.g_fwd_table is not None and not inv._loop.skip_uncond_fwd and not inv._loop.use_mask
    np.testing.assert_array_equal(inv._loop.g_fwd_table, np.linspace(2, 1, 1000))           # whatever guidance_scale_fwd says
    assert inv.get_timesteps_forward().tolist() == [0, 250, 500, 750]
    assert isinstance(inv.controller, ControllerEmpty) and inv._fast()
    inv.force_per_step = True
    assert not inv._fast()
    inv.force_per_step = False
    with inv.use_controller(ControllerBase()):
        assert not inv._fast()                                                             # a controller watches: the per-step path
    assert not modules.load_inverter("regdiffinv", model=_fake_model(), scheduler="dpm", num_inference_steps=4)._fast()
    with pytest.raises(ValueError, match="num_ac_rolls"):
        modules.load_inverter("regdiffinv", model=_fake_model(), num_inference_steps=4, num_ac_rolls=0)
    other = _fake_model()
    other.engine = types.SimpleNamespace(L=24, lib=None)
    from etainv.pipeline import EtaLoop
    with pytest.raises(ValueError, match="regulariser was built"):
        EtaLoop(other.engine, S=4, use_mask=False, regularizer=inv._reg)
    # losses: the reference's helpers, checked against the restatement with the same draws
    x = rr.multiscale_field(20, 1, seed=3).double()
    sh = rr.shift_table(20, 1, 1)
    got = inv.auto_corr_loss(x, generator=torch.Generator().manual_seed(0))
    np.testing.assert_allclose(float(got), float(rr.auto_corr_loss_torch(x[0], sh[0])), rtol=1e-12)
    fixed = np.ones((4, 3), dtype=np.int64)
    np.testing.assert_allclose(float(inv.auto_corr_loss(x, random_shift=False)), float(rr.auto_corr_loss_torch(x[0], fixed)), rtol=1e-12)
    np.testing.assert_allclose(float(inv.kl_divergence(x)), float(rr.kl_divergence_torch(x)), rtol=1e-12)
    with pytest.raises(ValueError, match="one image"):                                     # (the reference asserts a batch of one)
        inv.auto_corr_loss(torch.cat([x, x]))
    # the draws of one auto_corr_loss call are one autocorrelation step's rows of the shift table, at a size with three levels and an odd one
    np.testing.assert_array_equal(rr.shift_table(20, 1, 1), rr.shift_table(20)[:1])
