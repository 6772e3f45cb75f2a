"""Negative-prompt inversion on the native engine.  Plugin surface of the reference's modules/inversion/negative_prompt_inversion.py:8-31:
plain DDIM inversion whose backward pass puts the source prompt's conditional embedding in the place of the null embedding, on every
unconditional row, source and target alike (:20).

Two paths through the backward pass.  With an attention controller watching (ptp, masactrl), under a scheduler other than "ddim", or with
the attribute `force_per_step` set, every step is the base class's `predict_step_backward` (`_hooked_step`: controller hooks, UNet, CFG
kernel, scheduler kernel).  Otherwise a step is the UNet call and ONE etainv_prox_guidance launch (csrc/proximal.hip) that forms the guided
noise and takes the DDIM step -- in pass-through mode here, with the thresholding of proximal_negative_prompt_inversion.py in the subclass.

Deliberate deviation: the reference writes the embedding into the context tensor it was given (:20), so `sample` with a single tensor
overwrites the caller's context.  Here the write goes to a copy; the results are the same."""
from typing import Any, Dict, Optional

import torch

from etainv import _capi
from etainv.pipeline import ProximalGuidance
from .diffusion_inversion import DiffusionInversion


class NegativePromptInversion(DiffusionInversion):
    def __init__(self, model, scheduler: Optional[str] = None, num_inference_steps: Optional[int] = None,
                 guidance_scale_bwd: Optional[float] = None, guidance_scale_fwd: Optional[float] = None, verbose: bool = False) -> None:
        if getattr(model, "engine", None) is None:
            raise NotImplementedError(f"{type(self).__name__} needs a model on the native engine (model.engine, as load_diffusion_model builds it): its "
                                      "backward step is one etainv_prox_guidance launch; built inverters: etainv, dirinv, edict, regdiffinv, npi, "
                                      "proxnpi, diffinv")
        super().__init__(model, scheduler, num_inference_steps, guidance_scale_bwd, guidance_scale_fwd, verbose)
        self._ddim = self._plain_ddim(scheduler or None)        # the fused launch steps with the plain DDIM scheduler (a dict configures another one)
        self.L = model.engine.L
        self._guidance = self._make_guidance()

    def _make_guidance(self) -> ProximalGuidance:
        return ProximalGuidance(self.L, prox=None)

    def _both_halves(self, guidance_scale) -> bool:
        """the base class's predict_noise runs one half only at the scales 0 and 1; the fused step does what the per-step path does"""
        return not (isinstance(guidance_scale, (int, float)) and guidance_scale in (0, 1))

    # ------------------------------------------------------------------ one step
    def _guide(self, eps_u: torch.Tensor, eps_c: torch.Tensor, guidance_scale: float, x: Optional[torch.Tensor] = None, a_from: float = 1.0,
               a_to: float = 1.0, thr_out: Optional[torch.Tensor] = None):
        """etainv_prox_guidance over the rows of one call: they are one group, as the reference's quantile is taken over the whole tensor.
        fp32 inside; returns (noise, stepped latent or None) in the inputs' types"""
        if eps_u.shape != eps_c.shape or eps_u.dim() != 4 or tuple(eps_u.shape[1:]) != (4, self.L, self.L):
            raise ValueError(f"the two noise predictions must both be (rows, 4, {self.L}, {self.L}), got {tuple(eps_u.shape)} and {tuple(eps_c.shape)}")
        u, c = eps_u.detach().float().contiguous(), eps_c.detach().float().contiguous()
        out = torch.empty_like(c)
        xf = None if x is None else x.detach().float().contiguous()
        x_out = None if x is None else torch.empty_like(xf)
        self._guidance.run(_capi.load(), u, c, guidance_scale, out, xf, a_from, a_to, x_out, 1, u.shape[0], thr_out=thr_out)
        return out.to(eps_c.dtype), (None if x is None else x_out.to(x.dtype))

    def _fused_step(self, latent: torch.Tensor, t, context: torch.Tensor) -> torch.Tensor:
        """one backward step without hooks: the UNet call, then guidance and DDIM step in one launch"""
        g, n, rows = self.guidance_scale_bwd, latent.shape[0], context.shape[0]
        if rows == 2 * n and self._both_halves(g):
            eps = self.unet(latent.repeat(2, 1, 1, 1), t, encoder_hidden_states=context)["sample"]
            eps_u, eps_c = eps.chunk(2)
        elif rows == 2 * n:
            keep = slice(n, rows) if g == 1 else slice(0, n)
            eps_u = eps_c = self.unet(latent, t, encoder_hidden_states=context[keep])["sample"]          # d = 0: the noise passes unchanged
        else:
            raise AssertionError(f"the backward pass takes a context of [uncond rows, cond rows] over the latents: {n} latents, {rows} context rows")
        sched, t = self.scheduler_bwd, int(t)
        prev = t - sched.config.num_train_timesteps // sched.num_inference_steps
        return self._guide(eps_u, eps_c, g, latent, sched._alpha(t), sched._alpha(prev))[1]

    # ------------------------------------------------------------------ loops
    def _fast(self) -> bool:
        """the fused step serves the passes that no controller watches (force_per_step, an attribute, keeps the per-step path)"""
        return self._ddim and self._unwatched()

    def diffusion_backward(self, latent: torch.Tensor, context: torch.Tensor, inv_result: Dict[str, Any]) -> torch.Tensor:
        """(:17-23) at step i every unconditional row of the context is inv_result["uncond_embeddings"][i] -- in a copy of `context`"""
        context = context.clone()
        half = context.shape[0] // 2
        fast = self._fast()
        for i, t in enumerate(self.pbar(self.get_timesteps_backward(), desc="backward")):
            context[:half] = inv_result["uncond_embeddings"][i]
            if fast:
                latent = self._fused_step(latent, t, context)
            else:
                latent, _ = self.predict_step_backward(latent, t, context)
        return latent

    def invert(self, image: torch.Tensor, prompt: Optional[str] = None, context: Optional[torch.Tensor] = None,
               guidance_scale_fwd: Optional[float] = None, inv_cfg=None) -> Dict[str, Any]:
        """(:25-31) the base class's inversion; the conditional embedding is what the backward pass uses as null embedding at every step"""
        res = super().invert(image, prompt, context, guidance_scale_fwd)
        cond = res["context"].chunk(2)[1]
        res["uncond_embeddings"] = [cond] * self.num_inference_steps
        return res
