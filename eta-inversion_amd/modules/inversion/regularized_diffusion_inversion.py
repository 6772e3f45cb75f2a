"""Regularised DDIM inversion (pix2pix-zero) on the native engine.  Plugin surface of the reference's
modules/inversion/regularized_diffusion_inversion.py:11-137: plain DDIM inversion in which every guided noise prediction is pushed
towards white Gaussian noise before the scheduler step -- num_reg_steps rounds of num_ac_rolls gradient steps on an autocorrelation loss
over an average-pool pyramid and one gradient step on a KL term.  The reference takes both gradients from autograd; here they are
closed-form inside one kernel (csrc/regularize.hip, etainv_noise_regularize).  `invert` without an attention controller runs the batched
device loop `etainv.pipeline.EtaLoop` with a `NoiseRegularizer` (CFG combine, regularisation and DDIM step in one launch per step); the
per-step methods call the same kernel one step at a time.  The backward pass is the base class's."""
from typing import Optional, Tuple

import torch
import torch.nn.functional as F

from etainv import _capi
from etainv.pipeline import EtaLoop, NoiseRegularizer, regdiff_level_sizes
from .diffusion_inversion import DiffusionInversion


class RegularizedDiffusionInversion(DiffusionInversion):
    def __init__(self, model, scheduler: Optional[str] = None, num_inference_steps: Optional[int] = None,
                 guidance_scale_bwd: Optional[float] = None, guidance_scale_fwd: Optional[float] = None, verbose: bool = False,
                 lambda_ac: float = 20.0, lambda_kl: float = 20.0, num_reg_steps: int = 5, num_ac_rolls: int = 5) -> None:
        super().__init__(model, scheduler, num_inference_steps, guidance_scale_bwd, guidance_scale_fwd, verbose)
        if lambda_ac > 0 and num_reg_steps > 0 and num_ac_rolls <= 0:
            raise ValueError(f"num_ac_rolls must be positive when lambda_ac > 0, got {num_ac_rolls}")
        self.lambda_ac, self.lambda_kl, self.num_reg_steps, self.num_ac_rolls = lambda_ac, lambda_kl, num_reg_steps, num_ac_rolls
        self._ddim = not isinstance(scheduler, dict) and self._plain_ddim(scheduler or None)   # the batched loop steps with the plain DDIM inverse scheduler
        self.L = model.engine.L
        self._reg = NoiseRegularizer(self.L, lambda_ac, lambda_kl, num_reg_steps, num_ac_rolls, device=model.device)
        # forward guidance linspace(2, 1, 1000)[t], whatever scale is passed (:119-120)
        self._loop = EtaLoop(model.engine, S=self.num_inference_steps, guidance_scale_bwd=self.guidance_scale_bwd, guidance_scale_fwd=(2.0, 1.0),
                             use_mask=False, regularizer=self._reg)

    # ------------------------------------------------------------------ the two losses (plain torch; the kernel holds their gradients)
    def auto_corr_loss(self, x: torch.Tensor, random_shift: bool = True, generator: Optional[torch.Generator] = None) -> torch.Tensor:
        """L_ac of one image (1, C, s0, s0): over every channel and every level of its average-pool pyramid (sides `regdiff_level_sizes(s0)`), the
        squared autocorrelation at shift r along the rows plus the one along the columns, autocorrelation = mean(level * level rolled by r).
        r: one draw in [0, side // 2) per channel and level, channels outermost and levels from fine to coarse -- the order in which
        `regdiff_shift_table` draws -- or 1 everywhere without `random_shift`."""
        if x.dim() != 4 or x.shape[0] != 1:
            raise ValueError(f"auto_corr_loss takes one image (1, C, s, s), got {tuple(x.shape)}")
        sides = regdiff_level_sizes(x.shape[2])
        total = x.new_zeros(())
        for channel in x[0]:
            level = channel
            for k, side in enumerate(sides):
                if k > 0:
                    level = F.avg_pool2d(level[None, None], 2)[0, 0]
                r = int(torch.randint(0, side // 2, (), generator=generator)) if random_shift else 1
                for axis in (0, 1):
                    total = total + (level * level.roll(r, axis)).mean().square()
        return total

    def kl_divergence(self, x: torch.Tensor) -> torch.Tensor:
        """L_kl: the KL divergence (times two) of N(mean, variance) of all values from N(0, 1), unbiased variance, 1e-7 inside the logarithm"""
        variance, mean = torch.var_mean(x)
        return variance + mean.square() - 1 - (variance + 1e-7).log()

    # ------------------------------------------------------------------ one step
    def _regularize(self, noise_pred: torch.Tensor, shifts) -> torch.Tensor:
        if noise_pred.dim() != 4 or tuple(noise_pred.shape[1:]) != (4, self.L, self.L):
            raise ValueError(f"noise_pred must be (n, 4, {self.L}, {self.L}), got {tuple(noise_pred.shape)}")
        eps = noise_pred.detach().float().contiguous()
        out = torch.empty_like(eps)
        self._reg.run(_capi.load(), None, eps, 1.0, out, None, 1.0, 1.0, None, eps.shape[0], _capi.stream_ptr(), shifts=shifts)
        return out.to(noise_pred.dtype)

    def regularize_noise_pred(self, noise_pred: torch.Tensor, generator: Optional[torch.Generator] = None) -> torch.Tensor:
        """(:86-114) the roll amounts are drawn from `generator` (None: torch's global generator) on the host, in the reference's order, before
        the one launch; every image of a batch is regularised with the same draws (the reference holds exactly one image)"""
        return self._regularize(noise_pred, self._reg.table(generator if generator is not None else torch.default_generator))

    def predict_step_forward(self, latent: torch.Tensor, t: torch.Tensor, context: torch.Tensor,
                             guidance_scale_fwd: Optional[float] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """the base class's hooked forward step (`_hooked_step`) with the loop's guidance table in place of the scale that is passed (:119-120)
        and the regulariser between noise prediction and scheduler step; the reference reseeds its generator to 0 at every step (:117), so the
        draws are those of the loop's cached table"""
        g = float(self._loop.g_fwd_table[int(t)])
        latent = self.controller.begin_step(latent=latent)
        eps = self._regularize(self.predict_noise(latent, t, context, g, is_fwd=True), self._reg.table())
        stepped = self.step_forward(eps, t, latent).prev_sample
        return self.controller.end_step(latent=stepped, noise_pred=eps, t=t), eps

    # ------------------------------------------------------------------ loops
    def _fast(self) -> bool:
        """the batched device loop serves the passes that no controller watches (force_per_step, an attribute, keeps the per-step path)"""
        return self._ddim and self._unwatched()

    def diffusion_forward(self, latent, context, guidance_scale_fwd=None):
        n = latent.shape[0]
        if self._fast() and context.shape[0] == 2 * n:
            ctx = context.reshape(2, n, *context.shape[1:]).transpose(0, 1).float()      # rows [uncond x n, cond x n] -> (n, 2, 77, 768)
            res = self._loop.invert(latent.float().contiguous(), ctx)
            lat, eps = res["latents"], res["noise_preds"]
            trajectory = [lat[j] for j in range(lat.shape[0])]
            return {"latents": trajectory, "noise_preds": [eps[j] for j in range(eps.shape[0])], "zT_inv": trajectory[-1]}
        return super().diffusion_forward(latent, context, guidance_scale_fwd)
