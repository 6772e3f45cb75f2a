"""CPU-only checks of the `edict` inverter's host side: the native tables (coefficients, update order, truncated timesteps) against the
fixtures recorded from the reference implementation, the C ABI's refusals, the registry, and what the plugin layer refuses."""
import inspect
import types

import numpy as np
import pytest
import torch

from tests.golden.make_edict_golden import STEP_CASES


class _Engine:
    L = 16
    lib = None


@pytest.mark.parametrize("S,strength,leap", STEP_CASES)
def test_native_tables_match_reference(golden, S, strength, leap):
    from etainv.pipeline import EdictLoop
    g = golden("edict_steps")
    key = f"S{S}_s{strength}_l{int(leap)}"
    lp = EdictLoop(_Engine(), S=S, leapfrog_steps=leap, init_image_strength=strength)
    np.testing.assert_array_equal(lp.t_fwd, g[f"{key}/t_fwd"])
    np.testing.assert_array_equal(lp.t_bwd, g[f"{key}/t_bwd"])
    np.testing.assert_array_equal(np.array(lp.order_fwd), g[f"{key}/order_fwd"])
    np.testing.assert_array_equal(np.array(lp.order_bwd), g[f"{key}/order_bwd"])
    # coefficients are recorded over the full timestep lists; the loop's are the truncated ones
    n_f, n_b = len(lp.t_fwd), len(lp.t_bwd)
    np.testing.assert_allclose(np.array(lp.coef_fwd), g[f"S{S}/coef_fwd"][:n_f, :2], rtol=1e-6, atol=0)
    np.testing.assert_allclose(np.array(lp.coef_bwd), g[f"S{S}/coef_bwd"][S - n_b:, :2], rtol=1e-6, atol=0)


@pytest.mark.parametrize("S", [3, 4, 50])
def test_scheduler_wrappers_match_reference(golden, S):
    """EdictScheduler / EdictSchedulerInverse: timesteps, get_alpha_and_beta (fractional previous timestep at S = 3) and the step coefficients"""
    from modules.inversion.edict_inversion import EdictScheduler, EdictSchedulerInverse
    g = golden("edict_steps")
    for tag, cls in (("fwd", EdictSchedulerInverse), ("bwd", EdictScheduler)):
        sch = cls()
        sch.set_timesteps(S)
        np.testing.assert_array_equal(sch.timesteps.numpy(), g[f"S{S}/t_{tag}"])
        ref = g[f"S{S}/coef_{tag}"]
        for row, t in zip(ref, sch.timesteps):
            np.testing.assert_allclose(sch.coefficients(t), row[:2], rtol=1e-6, atol=0)
            np.testing.assert_allclose(float(sch.get_alpha_and_beta(t)[0]), row[2], rtol=1e-6)
            np.testing.assert_allclose(float(sch.get_alpha_and_beta(t - 1000 / S)[0]), row[3], rtol=1e-6)


def test_flops_entry_counts_two_unet_calls_per_step():
    from etainv.flops import edict_unet_rows
    from etainv.pipeline import EdictLoop
    assert edict_unet_rows(50, 50, 1, 2) == 2 * 50 * 2 + 2 * 50 * 4            # twice diffinv's 2 + 4 rows per step pair
    assert edict_unet_rows(3, 3, 2, 2, g_fwd=1.0) == 2 * 3 * 2 + 2 * 3 * 2 * 2 * 2
    lp = EdictLoop(_Engine(), S=5, init_image_strength=0.8)
    assert lp.expected_rows(B=1, n_prompts=2) == 2 * 4 * 2 + 2 * 4 * 4


def test_capi_refusals():
    """every bad call returns non-zero and leaves a message (the checks run before anything touches the device)"""
    from etainv import _capi
    lib = _capi.load()
    assert lib.etainv_abi_version() == 1
    p1, p2 = 4096, 8192                                                        # non-null stand-ins: refused calls never dereference
    err = lambda: lib.etainv_last_error().decode()
    assert lib.etainv_edict_couple(None, None, p1, 3.0, 1.0, 0.1, p2, 4, _capi.F32, None) != 0 and "null" in err()
    assert lib.etainv_edict_couple(p1, None, None, 3.0, 1.0, 0.1, p2, 4, _capi.F32, None) != 0 and "null" in err()
    assert lib.etainv_edict_couple(p1, None, p1, 3.0, 1.0, 0.1, p2, -1, _capi.F32, None) != 0 and "negative" in err()
    assert lib.etainv_edict_couple(p1, None, p1, 3.0, float("nan"), 0.1, p2, 4, _capi.F32, None) != 0 and "finite" in err()
    assert lib.etainv_edict_couple(p1, None, p1, 3.0, 1.0, 0.1, p2, 4, 7, None) != 0 and "dtype" in err()
    assert lib.etainv_edict_couple(p1, None, p1, 3.0, 1.0, 0.1, p2, 0, _capi.F32, None) == 0      # n == 0: nothing to do
    assert lib.etainv_edict_mix(None, p2, 0.93, 0, 4, _capi.F32, None) != 0 and "null" in err()
    assert lib.etainv_edict_mix(p1, p1, 0.93, 0, 4, _capi.F32, None) != 0 and "pair" in err()
    for p in (0.0, -0.5, 1.5, float("nan")):
        assert lib.etainv_edict_mix(p1, p2, p, 0, 4, _capi.F32, None) != 0 and "(0, 1]" in err()
        assert lib.etainv_edict_couple_mix(p1, p2, 0, None, p1, 3.0, 1.0, 0.1, p, 4, _capi.F32, None) != 0 and "(0, 1]" in err()
    assert lib.etainv_edict_mix(p1, p2, 0.93, 2, 4, _capi.F32, None) != 0 and "inverse" in err()
    assert lib.etainv_edict_mix(p1, p2, 1.0, 1, 0, _capi.F32, None) == 0
    assert lib.etainv_edict_couple_mix(p1, None, 0, None, p1, 3.0, 1.0, 0.1, 0.93, 4, _capi.F32, None) != 0 and "null" in err()
    assert lib.etainv_edict_couple_mix(p1, p2, 2, None, p1, 3.0, 1.0, 0.1, 0.93, 4, _capi.F32, None) != 0 and "base_is_y" in err()
    assert lib.etainv_edict_couple_mix(p1, p2, 1, None, p1, 3.0, 1.0, 0.1, 0.93, 4, 9, None) != 0 and "dtype" in err()
    with pytest.raises(_capi.EtainvError):
        _capi.check(lib.etainv_edict_mix(p1, p2, 0.0, 0, 4, _capi.F32, None))


def test_registry_and_signature():
    import modules
    from modules.inversion.edict_inversion import EdictInversion, EdictScheduler, EdictSchedulerInverse
    from modules.editing.controller import EdictController
    assert "edict" in modules.get_inversion_methods()
    assert modules._inverters["edict"] is EdictInversion and issubclass(EdictInversion, modules.DiffusionInversion)
    sig = inspect.signature(EdictInversion.__init__).parameters
    assert list(sig)[1:] == ["model", "scheduler", "num_inference_steps", "guidance_scale_bwd", "guidance_scale_fwd", "verbose", "mix_weight",
                             "leapfrog_steps", "init_image_strength", "prec"]
    assert (sig["mix_weight"].default, sig["leapfrog_steps"].default, sig["init_image_strength"].default) == (0.93, True, 1.0)
    assert (EdictInversion.dft_mix_weight, EdictInversion.dft_leapfrog_steps, EdictInversion.dft_init_image_strength) == (0.93, True, 0.8)
    for name in ("encode", "decode", "cat_latent", "iter_latent_pair", "sync_latent_pair", "predict_step_forward", "predict_step_backward",
                 "predict_step_forward_single", "predict_step_backward_single", "get_timesteps_forward", "get_timesteps_backward", "use_controller"):
        assert name in vars(EdictInversion), name
    assert EdictSchedulerInverse.inverse and not EdictScheduler.inverse and callable(EdictController)
    with pytest.raises(NotImplementedError) as e:                          # the message of what is still missing names what exists
        modules.load_inverter("nti", model=None)
    assert "edict" in str(e.value)


def _fake_model():
    from modules.schedulers import DDIMScheduler
    sched = DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", clip_sample=False, set_alpha_to_one=False)
    return types.SimpleNamespace(unet=None, device="cpu", scheduler=sched, engine=_Engine())


def test_plugin_tables_and_refusals():
    """what the constructor builds without touching the device, and what the plugin layer refuses"""
    import modules
    from modules.editing.controller import ControllerBase, ControllerEmpty, EdictController
    from modules.editing.masactrl_editor import MasactrlController
    with pytest.raises(NotImplementedError, match="dpm"):
        modules.load_inverter("edict", model=_fake_model(), scheduler="dpm", num_inference_steps=4)
    with pytest.raises(ValueError):
        modules.load_inverter("edict", model=_fake_model(), num_inference_steps=4, mix_weight=0.0)
    inv = modules.load_inverter("edict", model=_fake_model(), num_inference_steps=5, init_image_strength=0.8)
    assert (inv.guidance_scale_fwd, inv.guidance_scale_bwd, inv.mix_weight, inv.t_limit) == (3.0, 3.0, 0.93, 1)
    assert inv.get_timesteps_forward().tolist() == [0, 200, 400, 600] and inv.get_timesteps_backward().tolist() == [600, 400, 200, 0]
    assert inv.fwd_t_to_i == {0: 0, 200: 1, 400: 2, 600: 3} and inv.bwd_t_to_i == {600: 0, 400: 1, 200: 2, 0: 3}
    pair = ["x", "y"]
    assert [k for k, _ in inv.iter_latent_pair(0, pair, is_fwd=True)] == list(inv._loop.order_fwd[0])
    assert [k for k, _ in inv.iter_latent_pair(1, pair, is_fwd=False)] == [1, 0]
    assert isinstance(inv.controller, EdictController) and all(isinstance(c, ControllerEmpty) for c in inv.controller.controllers)

    # a controller without copy() -- MasaCtrl, a user controller -- is not built
    class Custom(ControllerBase):
        pass
    for ctl in (Custom(), MasactrlController(4, 10)):
        with pytest.raises(NotImplementedError, match="copy"):
            with inv.use_controller(ctl):
                pass

    # prompt-to-prompt with LocalBlend: its copies would blend from one store that both pair members wrote
    class WithBlend(ControllerBase):
        def __init__(self, blend):
            self.controller = types.SimpleNamespace(local_blend=blend)

        def copy(self, **kwargs):
            return WithBlend(self.controller.local_blend)
    with pytest.raises(NotImplementedError, match="needs a per-latent map store"):
        EdictController(WithBlend(object()))
    two = EdictController(WithBlend(None))
    assert len(two.controllers) == 2 and two.controllers[0] is not two.controllers[1]


def test_ptp_controller_with_blend_words_is_refused():
    """the real PromptToPromptController: with blend_words its copies carry a LocalBlend -> refused; without, two independent copies"""
    from modules.editing.controller import EdictController
    from modules.editing.ptp_editor import PromptToPromptController
    from modules.utils.tokenizer import WordLevelTokenizer
    src, tgt = "a cat sitting next to a mirror", "a tiger sitting next to a mirror"
    model = _fake_model()
    model.tokenizer = WordLevelTokenizer()
    model.scheduler.set_timesteps(4)
    cfg = dict(is_replace_controller=False, cross_replace_steps={"default_": .4}, self_replace_steps=0.6)
    with pytest.raises(NotImplementedError, match="needs a per-latent map store"):
        EdictController(PromptToPromptController(model, src, tgt, blend_words=(("cat",), ("tiger",)), **cfg))
    pair = EdictController(PromptToPromptController(model, src, tgt, **cfg))
    assert pair.controllers[0] is not pair.controllers[1] and pair.controllers[0].controller.local_blend is None
