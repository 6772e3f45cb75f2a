"""Inverse DDPM scheduler of edit-friendly DDPM inversion (reference modules/inverse_schedulers/ddpm_inverse_scheduler.py:9-203): same
constructor, `from_scheduler`, `set_timesteps`, `timesteps`, `get_variance`, `sample_latents`, `get_sampled_latent_by_t`, `get_eta_by_t` and
`step -> Output(prev_sample, variance_noise)`.  `sample_latents` noises the latent to every timestep in one etainv_ddpm_sample_latents launch;
`step` turns a noise prediction into the step's noise map and corrected latent in one etainv_ddpm_invert_steps launch (csrc/ddpm.hip).  All
schedule coefficients are float64 host scalars (etainv.pipeline.ddpm_*).

`sample_latents` draws with torch.randn on the latent's device like the reference, one draw per timestep in ascending t; the additional
keyword `noise` takes those draws, [S][1][4][L][L], from the caller instead (a ROCm generator's stream is not the CPU generator's).

Deliberate deviation: at sigma == 0 (t = 0 under steps_offset = 0) the reference divides by zero (:193) and returns NaN; here the noise map is
0 and the corrected latent is mu.  DDPMInversion zeroes that map anyway and never reads that latent (ddpm_inversion.py:101)."""
from collections import namedtuple
from typing import Optional

import numpy as np
import torch

from etainv import _capi
from etainv.pipeline import (ddpm_invert_steps, ddpm_sample_coefficients, ddpm_sample_latents, ddpm_step_coefficients, ddpm_variance)
from ..schedulers import DDIMScheduler
from .diffusion_inverse_scheduler import DiffusionInverseScheduler


class DDPMInverseScheduler(DiffusionInverseScheduler):
    Output = namedtuple("DDPMInverseSchedulerOutput", ("prev_sample", "variance_noise"))

    def __init__(self, scheduler: DDIMScheduler, inv_steps: str = "sameshift", eta: int = 1, markovian_forward=False) -> None:
        self.scheduler = scheduler
        self.inv_steps = inv_steps
        self.etas = None
        self.t_to_idx = None
        self.markovian_forward = markovian_forward

    @staticmethod
    def from_scheduler(scheduler, inv_steps="sameshift", markovian_forward=False, **kwargs) -> "DDPMInverseScheduler":
        return DDPMInverseScheduler(DDIMScheduler.from_config({**scheduler.config, **kwargs}), inv_steps=inv_steps,
                                    markovian_forward=markovian_forward)

    def set_timesteps(self, num_inference_steps: int) -> None:
        self.scheduler.set_timesteps(num_inference_steps)
        self.t_to_idx = {int(v): k for k, v in enumerate(self.scheduler.timesteps)}
        self.etas = [1.0] * num_inference_steps
        ac = self._ac = self.scheduler.alphas_cumprod.double().numpy()
        final, S = float(self.scheduler.final_alpha_cumprod), num_inference_steps
        self._coef = np.stack([ddpm_step_coefficients(ac, final, S, t) for t in self.scheduler.timesteps])          # by xts index

    @property
    def timesteps(self) -> torch.Tensor:
        return torch.flip(self.scheduler.timesteps, dims=(0,))

    def get_variance(self, timestep: int) -> float:
        """(:65-84) in float64"""
        return ddpm_variance(self._ac, float(self.scheduler.final_alpha_cumprod), self.scheduler.num_inference_steps, int(timestep))

    def sample_latents(self, latent: torch.Tensor, generator: Optional[torch.Generator] = None, noise: Optional[torch.Tensor] = None) -> torch.Tensor:
        """(:86-129) latent (1,4,L,L) -> all noised latents and the latent itself, (S+1,4,L,L): index 0 = the largest timestep, index S = latent"""
        S = len(self.timesteps)
        if latent.dim() != 4 or latent.shape[0] != 1:
            raise ValueError(f"sample_latents noises one latent (1,4,L,L) (the reference's torch.cat takes no other), got {tuple(latent.shape)}")
        if noise is None:
            noise = torch.stack([torch.randn(latent.shape, device=latent.device, generator=generator).to(latent.dtype) for _ in range(S)])
        elif tuple(noise.shape) != (S, *latent.shape):
            raise ValueError(f"noise must hold one draw per timestep, {(S, *latent.shape)}, got {tuple(noise.shape)}")
        ab = ddpm_sample_coefficients(self._ac, S, self.markovian_forward, timesteps=self.timesteps)
        xts = ddpm_sample_latents(_capi.load(), latent.float().contiguous(), noise.to(latent.device).float().contiguous(), ab, self.markovian_forward)
        return xts[:, 0].to(latent.dtype)

    def get_sampled_latent_by_t(self, xts: torch.Tensor, t: int) -> torch.Tensor:
        return xts[self.t_to_idx[int(t)]][None]

    def get_eta_by_t(self, t: int) -> float:
        return self.etas[self.t_to_idx[int(t)]]

    def step(self, noise_pred: torch.Tensor, t: int, latent: torch.Tensor, xts: torch.Tensor) -> "DDPMInverseScheduler.Output":
        """(:156-199) `latent` is unused, as in the reference: x_t and x_{t-1} are read from xts.  One k = 1 launch."""
        idx = self.t_to_idx[int(t)]
        x = xts.float().contiguous()[:, None]
        eps = noise_pred.float().contiguous()
        z, out = torch.empty_like(eps), torch.empty_like(eps)
        ddpm_invert_steps(_capi.load(), x, idx, 1, None, eps, 1.0, self._coef[idx:idx + 1], z, out, None)
        return DDPMInverseScheduler.Output(out.to(noise_pred.dtype), z.to(noise_pred.dtype))
