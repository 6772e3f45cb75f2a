"""CPU-only checks of the `npi` / `proxnpi` inverters' host side: the registry, the constructors' signatures and defaults, the refusals made
before anything touches the device (the C ABI's and the plugins'), and construction on a fake model."""
import inspect
import types

import pytest
import torch

BASE = ["model", "scheduler", "num_inference_steps", "guidance_scale_bwd", "guidance_scale_fwd", "verbose"]


class _Engine:
    L = 16
    lib = None


def _fake_model():
    from modules.schedulers import DDIMScheduler
    sched = DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", clip_sample=False, set_alpha_to_one=False)
    return types.SimpleNamespace(unet=None, device="cpu", scheduler=sched, engine=_Engine())


def test_registry_and_signatures():
    import modules
    from modules.editing.inv_editor import InversionEditor
    from modules.inversion.negative_prompt_inversion import NegativePromptInversion
    from modules.inversion.proximal_negative_prompt_inversion import ProximalNegativePromptInversion
    assert {"npi", "proxnpi"} <= set(modules.get_inversion_methods()) and "invedit" in modules.get_edit_methods()
    assert modules._inverters["npi"] is NegativePromptInversion and modules._inverters["proxnpi"] is ProximalNegativePromptInversion
    assert modules._editors["invedit"] is InversionEditor and issubclass(InversionEditor, modules.Editor)
    assert issubclass(ProximalNegativePromptInversion, NegativePromptInversion) and issubclass(NegativePromptInversion, modules.DiffusionInversion)
    assert list(inspect.signature(NegativePromptInversion.__init__).parameters)[1:] == BASE
    sig = inspect.signature(ProximalNegativePromptInversion.__init__).parameters
    assert list(sig)[1:] == BASE + ["prox", "quantile", "recon_lr", "recon_t", "dilate_mask"]
    assert [sig[n].default for n in ("prox", "quantile", "recon_lr", "recon_t", "dilate_mask")] == ["l0", 0.7, 1, 400, 1]
    P = ProximalNegativePromptInversion
    assert (P.dft_prox, P.dft_quantile, P.dft_recon_lr, P.dft_recon_t, P.dft_dilate_mask) == ("l0", 0.7, 1, 400, 1)
    assert list(inspect.signature(NegativePromptInversion.invert).parameters)[1:] == ["image", "prompt", "context", "guidance_scale_fwd", "inv_cfg"]
    assert list(inspect.signature(NegativePromptInversion.diffusion_backward).parameters)[1:] == ["latent", "context", "inv_result"]
    assert list(inspect.signature(P.proximal_guidance).parameters)[1:] == ["noise_pred_uncond", "noise_prediction_text", "t", "guidance_scale"]
    assert list(inspect.signature(P.predict_noise).parameters)[1:] == ["latent", "t", "context", "guidance_scale", "is_fwd", "kwargs"]
    assert list(inspect.signature(InversionEditor.__init__).parameters)[1:] == ["inverter", "no_source_backward", "vae_rec", "no_null_source_prompt"]
    assert not hasattr(__import__("modules.inversion.proximal_negative_prompt_inversion", fromlist=["x"]), "_dilate")       # dead in the reference
    from etainv import _capi
    assert len(_capi.SIGNATURES["etainv_prox_guidance"]) == 18 and hasattr(_capi.load(), "etainv_prox_guidance")
    assert _capi.load().etainv_abi_version() == 1


def test_what_is_still_not_built():
    import modules
    for name in ("nti", "ddpminv", "cyclediff"):
        with pytest.raises(NotImplementedError, match="npi, proxnpi") as e:
            modules.load_inverter(name, model=None)
        assert "edict" in str(e.value) and "regdiffinv" in str(e.value) and "simple, ptp, masactrl, pnp" in str(e.value)
    with pytest.raises(NotImplementedError, match="invedit"):
        modules.load_editor("pix2pix_zero", inverter=None)
    # a model without an engine: refused first, with what the inverter needs and what is built
    for name in ("npi", "proxnpi"):
        with pytest.raises(NotImplementedError, match="model.engine") as e:
            modules.load_inverter(name, model=None)
        assert "regdiffinv" in str(e.value) and "npi, proxnpi" in str(e.value) and "etainv_prox_guidance" in str(e.value)
        with pytest.raises(NotImplementedError, match="model.engine"):
            modules.load_inverter(name, model=types.SimpleNamespace(unet=None, device="cpu"))


def test_construction_and_refusals():
    import modules
    from etainv.pipeline import ProximalGuidance
    from modules.editing.controller import ControllerBase, ControllerEmpty
    npi = modules.load_inverter("npi", model=_fake_model(), num_inference_steps=4)
    assert isinstance(npi._guidance, ProximalGuidance) and npi._guidance.prox is None and npi.L == 16
    assert (npi.guidance_scale_bwd, npi.guidance_scale_fwd) == (7.5, 1)
    assert npi.get_timesteps_backward().tolist() == [750, 500, 250, 0]
    assert isinstance(npi.controller, ControllerEmpty) and npi._fast()
    npi.force_per_step = True
    assert not npi._fast()
    npi.force_per_step = False
    with npi.use_controller(ControllerBase()):
        assert not npi._fast()                                                             # a controller watches: the per-step path
    assert not modules.load_inverter("npi", model=_fake_model(), scheduler="dpm", num_inference_steps=4)._fast()
    assert not npi._both_halves(1) and not npi._both_halves(0) and npi._both_halves(7.5)   # the base class's shortcut, as on the per-step path
    prox = modules.load_inverter("proxnpi", model=_fake_model(), num_inference_steps=4, recon_t=-300, recon_lr=2, dilate_mask=0)
    assert (prox.prox, prox.quantile, prox.recon_t, prox.recon_lr, prox.dilate_mask) == ("l0", 0.7, -300, 2, 0)
    assert (prox._guidance.prox, prox._guidance.quantile, prox._guidance.L) == ("l0", 0.7, 16)
    assert prox._both_halves(1) and prox._both_halves(0) and prox._fast()                  # never the shortcut
    fixed = modules.load_inverter("proxnpi", model=_fake_model(), num_inference_steps=4, prox="l1", quantile=-0.25)
    assert (fixed._guidance.prox, fixed._guidance.quantile) == ("l1", -0.25)
    assert modules.load_inverter("proxnpi", model=_fake_model(), quantile=1.0).quantile == 1.0
    for q in (1.0001, 2, 70):
        with pytest.raises(ValueError, match="quantile"):
            modules.load_inverter("proxnpi", model=_fake_model(), quantile=q)
        with pytest.raises(ValueError, match="quantile"):
            ProximalGuidance(16, quantile=q)
    # an unknown prox is accepted by the constructor and refused at the call, as in the reference
    l2 = modules.load_inverter("proxnpi", model=_fake_model(), num_inference_steps=4, prox="l2")
    eps = torch.zeros(2, 4, 16, 16)
    with pytest.raises(NotImplementedError, match="l2"):
        l2.proximal_guidance(eps, eps, torch.tensor(500), 7.5)
    with pytest.raises(ValueError, match=r"\(rows, 4, 16, 16\)"):
        prox.proximal_guidance(torch.zeros(2, 4, 8, 8), torch.zeros(2, 4, 8, 8), 500, 7.5)
    # invert adds the conditional embedding, once per step (the same tensor every time)
    ctx = torch.randn(2, 77, 768)
    npi.encode = lambda image: image
    npi.diffusion_forward = lambda latent, context, guidance_scale_fwd=None: {"latents": [latent], "noise_preds": [], "zT_inv": latent}
    res = npi.invert(torch.zeros(1, 4, 16, 16), context=ctx, inv_cfg={"unused": 1})
    assert len(res["uncond_embeddings"]) == 4 and all(torch.equal(e, ctx[1:2]) for e in res["uncond_embeddings"]) and res["context"] is ctx


def _call(lib, **over):
    """etainv_prox_guidance with plausible arguments (non-null stand-in pointers: refused calls never dereference), overridden by name"""
    a = dict(eps_u=4096, eps_c=8192, g=7.5, mode=1, use_rank=1, rank_lo=100, rank_w=0.5, thr_fixed=0.0, eps_out=12288, x=None, a_from=0.9, a_to=0.8,
             x_out=None, thr_out=None, n_groups=1, rows_per_group=2, l=16)
    a.update(over)
    return lib.etainv_prox_guidance(a["eps_u"], a["eps_c"], a["g"], a["mode"], a["use_rank"], a["rank_lo"], a["rank_w"], a["thr_fixed"], a["eps_out"],
                                    a["x"], a["a_from"], a["a_to"], a["x_out"], a["thr_out"], a["n_groups"], a["rows_per_group"], a["l"], None)


def test_capi_refusals():
    from etainv import _capi
    lib = _capi.load()
    err = lambda: lib.etainv_last_error().decode()
    nan, inf = float("nan"), float("inf")
    n = 2 * 4 * 16 * 16
    refused = [
        (dict(eps_u=None), "null pointer"), (dict(eps_c=None), "null pointer"), (dict(eps_out=None), "null pointer"),
        (dict(eps_out=4096), "not eps_u"),
        (dict(x=4096), "x_out"),
        (dict(mode=3), "mode"), (dict(mode=-1), "mode"),
        (dict(l=7), "[8, 96]"), (dict(l=97), "[8, 96]"), (dict(l=0), "[8, 96]"),
        (dict(rows_per_group=5), "[1, 4]"), (dict(rows_per_group=0), "[1, 4]"),
        (dict(n_groups=-1), "negative"),
        (dict(g=nan), "g must be finite"), (dict(g=inf), "g must be finite"),
        (dict(a_from=nan), "finite"), (dict(a_to=inf), "finite"),
        (dict(x=4096, x_out=8192, a_from=0.0), "(0,1]"), (dict(x=4096, x_out=8192, a_to=1.5), "(0,1]"),
        (dict(rank_lo=-1), "[0, n - 1]"), (dict(rank_lo=n), "[0, n - 1]"), (dict(mode=2, rank_lo=n + 5), "[0, n - 1]"),
        (dict(rank_w=1.0), "[0, 1)"), (dict(rank_w=-0.1), "[0, 1)"), (dict(rank_w=nan), "[0, 1)"),
        (dict(use_rank=0, thr_fixed=-0.5), "fixed threshold"), (dict(use_rank=0, thr_fixed=nan), "fixed threshold"),
    ]
    for over, fragment in refused:
        assert _call(lib, **over) != 0, over
        assert fragment in err() and "etainv_prox_guidance" in err(), (over, err())
    with pytest.raises(_capi.EtainvError, match="x_out"):
        _capi.check(_call(lib, x=4096))
    # n_groups == 0: nothing to do; plain CFG ignores the rank and the threshold; the last rank is a rank
    assert _call(lib, n_groups=0) == 0 and _call(lib, n_groups=0, rank_lo=n - 1, rank_w=0.0) == 0
    assert _call(lib, n_groups=0, mode=0, rank_lo=-7, rank_w=nan, thr_fixed=nan) == 0
    assert _call(lib, n_groups=0, l=8, rows_per_group=1, rank_lo=255) == 0 and _call(lib, n_groups=0, l=96, rows_per_group=4, rank_lo=147455) == 0
