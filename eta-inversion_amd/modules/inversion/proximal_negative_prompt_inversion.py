"""Proximal negative-prompt inversion on the native engine.  Plugin surface of the reference's
modules/inversion/proximal_negative_prompt_inversion.py:23-151: negative-prompt inversion whose backward pass thresholds the guidance term
d = eps_c - eps_u at a quantile of its magnitudes before it is scaled (:61-128).  Threshold, shrinkage, guided noise and -- on the fused path of
negative_prompt_inversion.py -- the DDIM step are one launch, etainv_prox_guidance (csrc/proximal.hip): the quantile is an exact selection of
the two order statistics torch.quantile interpolates between, not a sort.

What the reference computes, kept as it is:
  * the quantile is over the whole tensor of the call (:85,105).  In an edit that is the source and the target row; the source pair's
    unconditional and conditional rows see the same latent and the same context, so its d is zero and fills the low ranks: at quantile 0.7 the
    threshold is the 0.4-quantile of the target row's |d|;
  * "l0" is soft shrinkage, d - clamp(d, -thr, thr) (:108); "l1" shrinks once more with two `where`s in sequence (:88-90), which is not
    symmetric: with thr = 1, d = -1.5 gives +0.5 and d = 2 gives 0 (jumps at d = -thr and d = 2 thr).

What is not rebuilt: the recon_t / recon_lr / dilate_mask branch (:91-98, :109-116) builds a mask into `step_kwargs`, and :123-126 delete
every entry of `step_kwargs` before the return, so the branch has no effect on any result.  The three parameters are accepted and stored; no
mask is computed, and `_dilate` (:10-20) does not exist here.

Deviation: the reference in fp16 forms d in fp16 (:83,100).  Here the engine's noise is fp32, and inputs of another type are converted: d is
always formed in fp32; the result is returned in the input's type."""
from typing import Optional, Union

import torch

from etainv.pipeline import ProximalGuidance
from .negative_prompt_inversion import NegativePromptInversion


class ProximalNegativePromptInversion(NegativePromptInversion):
    dft_prox = "l0"
    dft_quantile = 0.7
    dft_recon_lr = 1
    dft_recon_t = 400
    dft_dilate_mask = 1

    def __init__(self, model, scheduler: Optional[str] = None, num_inference_steps: Optional[int] = None,
                 guidance_scale_bwd: Optional[float] = None, guidance_scale_fwd: Optional[float] = None, verbose: bool = False,
                 prox: str = "l0", quantile: float = 0.7, recon_lr: int = 1, recon_t: int = 400, dilate_mask: int = 1) -> None:
        if quantile > 1:
            raise ValueError(f"quantile must be at most 1 (a quantile of |eps_c - eps_u|) or <= 0 (a fixed threshold), got {quantile}")
        self.prox, self.quantile = prox, quantile
        self.recon_t, self.recon_lr, self.dilate_mask = recon_t, recon_lr, dilate_mask
        super().__init__(model, scheduler, num_inference_steps, guidance_scale_bwd, guidance_scale_fwd, verbose)

    def _make_guidance(self) -> ProximalGuidance:
        return ProximalGuidance(self.L, prox=self.prox, quantile=self.quantile)

    def _both_halves(self, guidance_scale) -> bool:
        """the threshold needs both halves at every scale (:142-147): at scale 1 the result is eps_u + d', not eps_c"""
        return True

    def proximal_guidance(self, noise_pred_uncond: torch.Tensor, noise_prediction_text: torch.Tensor, t, guidance_scale: float) -> torch.Tensor:
        """(:61-128) eps_u + guidance_scale * shrink(eps_c - eps_u); the rows of the call share one threshold.  `t` only selects the reference's
        dead mask branch and is not used."""
        return self._guide(noise_pred_uncond, noise_prediction_text, guidance_scale)[0]

    def predict_noise(self, latent: torch.Tensor, t, context: torch.Tensor, guidance_scale: Union[float, int, None], is_fwd: bool = False,
                      **kwargs) -> torch.Tensor:
        """(:130-151) the forward pass and guidance None are the base class's; the backward pass always runs both halves"""
        if guidance_scale is None or is_fwd:
            return super().predict_noise(latent, t, context, guidance_scale, is_fwd=is_fwd, **kwargs)
        if latent.shape[0] * 2 == context.shape[0]:
            latent = latent.repeat(2, *([1] * (latent.dim() - 1)))
        assert latent.shape[0] == context.shape[0]
        eps_u, eps_c = self.unet(latent, t, encoder_hidden_states=context, **kwargs)["sample"].chunk(2)
        return self.proximal_guidance(eps_u, eps_c, t, guidance_scale)
