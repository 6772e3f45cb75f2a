"""Edit-friendly DDPM inversion on the native engine.  Plugin surface of the reference's modules/inversion/ddpm_inversion.py:10-177: the image
latent is noised to every timestep at once (DDPMInverseScheduler.sample_latents), each step's noise map z is what makes the DDPM step from x_t
land on the sampled x_{t-1}, and the backward pass replays the maps as the variance noise of DDIM steps at eta = 1, the source row under
guidance_scale_fwd and the target row under guidance_scale_bwd.  `cyclediff` is this class with markovian_forward=True.

Two paths through the inversion.  The reference runs S UNet calls one after the other, but nothing in them is sequential: every x_t exists
before the first call.  Outside a controller (editors always invert there) the steps go to the UNet in chunks of whole steps with one
timestep per row -- max_unet_batch // 2 steps per call, max_unet_batch when the scale is 0 or 1 -- each followed by ONE
etainv_ddpm_invert_steps launch (etainv.pipeline.DdpmLoop.invert with B = 1).  With the attribute `force_per_step` set, or a controller
watching, it is the reference's loop: `predict_step_forward` per step, one UNet call and one k = 1 launch.  The two paths agree to rounding,
not to the bit: the engine picks kernel forms from a call's row count.

Two paths through the backward pass.  Unwatched: per step one UNet call and ONE etainv_ddpm_backward_step launch (DdpmLoop.backward).  Under a
controller (ptp, masactrl): `predict_step_backward` per step -- hooks, UNet, etainv_cfg_combine per prompt row, etainv_ddim_eta_step.  The
prompt-to-prompt controller counts its steps from 0 although the loop starts behind the skipped steps, as in the reference.

`forward_noise` (attribute, default None): the [S][1][4][L][L] draws of sample_latents, ascending t, instead of the seeded generator's.

Deliberate deviations.
  sigma == 0   at t = 0 the reference divides by zero (ddpm_inverse_scheduler.py:193): its noise map and latent are NaN there.  Here the map is
               0 and the latent is mu.  The reference zeroes that map afterwards (:101) and never reads that latent.
  skip == 0    int(skip_steps * S) == 0 (a small S, or skip_steps tiny) turns the reference's `[:-0]` slices into empty lists and `sample` fails;
               here a skip of 0 skips nothing: the backward pass runs all S steps from the noisiest latent."""
from typing import Any, Dict, List, Optional, Tuple, Union

import torch

from etainv.pipeline import DdpmLoop
from ..inverse_schedulers import DDPMInverseScheduler
from ..schedulers import DDIMScheduler
from .diffusion_inversion import DiffusionInversion


class DDPMInversion(DiffusionInversion):
    dft_skip_steps = 0.36
    dft_forward_seed = 0

    def __init__(self, model, scheduler: Optional[str] = None, num_inference_steps: Optional[int] = None,
                 guidance_scale_bwd: Optional[float] = None, guidance_scale_fwd: Optional[float] = None, verbose: bool = False,
                 forward_seed: Optional[int] = 0, skip_steps: Optional[float] = None, markovian_forward: bool = False) -> None:
        if getattr(model, "engine", None) is None:
            raise NotImplementedError(f"{type(self).__name__} needs a model on the native engine (model.engine, as load_diffusion_model builds it): its "
                                      "steps are etainv_ddpm_invert_steps / etainv_ddpm_backward_step launches; built inverters: etainv, dirinv, edict, "
                                      "regdiffinv, npi, proxnpi, ddpminv, cyclediff, diffinv; built editors: simple, ptp, masactrl, pnp, invedit")
        guidance_scale_fwd = guidance_scale_fwd or 3.5
        guidance_scale_bwd = guidance_scale_bwd or 9
        self.skip_steps = skip_steps or 0.36
        self.forward_seed = forward_seed if forward_seed >= 0 else None
        self.markovian_forward = markovian_forward
        self.forward_noise = None
        super().__init__(model, "ddpm", num_inference_steps, guidance_scale_bwd, guidance_scale_fwd, verbose)   # (the scheduler is forced, :36,46)
        self.L = model.engine.L
        self._loop = DdpmLoop(model.engine, S=self.num_inference_steps, guidance_scale_fwd=self.guidance_scale_fwd,
                              guidance_scale_bwd=self.guidance_scale_bwd, skip_steps=self.skip_steps, markovian_forward=markovian_forward)

    def create_schedulers(self, model, scheduler, num_inference_steps, scheduler_inv_kwargs=None) -> Tuple[DDIMScheduler, DDIMScheduler, DDPMInverseScheduler]:
        """(:45-46 with diffusion_inversion.py:139-172) backward: the DDIM scheduler under the model's own configuration (the reference adds its
        clip_sample / set_alpha_to_one defaults for the name "ddim" only); forward: the DDPM inverse scheduler over a copy of it"""
        sched = DDIMScheduler.from_config({**model.scheduler.config})
        sched.set_timesteps(num_inference_steps)
        fwd = DDPMInverseScheduler.from_scheduler(sched, markovian_forward=self.markovian_forward, **dict(scheduler_inv_kwargs or {}))
        fwd.set_timesteps(num_inference_steps)
        assert fwd.timesteps[0] < fwd.timesteps[-1] or num_inference_steps == 1, "wrong timestamp order, not increasing"
        return sched, sched, fwd

    # ------------------------------------------------------------------ inversion
    def predict_step_forward(self, latent, t, context, guidance_scale_fwd, xts) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(:48-69) -> (corrected latent, noise prediction, noise map)"""
        guidance_scale_fwd = guidance_scale_fwd or self.guidance_scale_fwd
        noise_pred = self.predict_noise(latent, t, context, guidance_scale_fwd, is_fwd=False)
        res = self.step_forward(noise_pred, t, latent, xts)
        return res.prev_sample, noise_pred, res.variance_noise

    def _draw(self, latent: torch.Tensor) -> torch.Tensor:
        """the S draws of sample_latents (ddpm_inverse_scheduler.py:114) from the seeded generator on the latent's device (:74), or `forward_noise`"""
        S = self.num_inference_steps
        if self.forward_noise is not None:
            noise = self.forward_noise.to(latent.device).float()
            if tuple(noise.shape) != (S, *latent.shape):
                raise ValueError(f"forward_noise must be {(S, *latent.shape)}, one draw per timestep in ascending t, got {tuple(noise.shape)}")
            return noise
        gen = torch.Generator(latent.device).manual_seed(self.forward_seed) if self.forward_seed is not None else None
        return torch.stack([torch.randn(latent.shape, device=latent.device, generator=gen).to(latent.dtype) for _ in range(S)])

    def _fast(self) -> bool:
        """the time-parallel inversion and the fused backward step serve the passes that no controller watches (force_per_step, an attribute,
        keeps the per-step path)"""
        cfg = self.scheduler_bwd.config          # (the loop's tables are those of steps_offset 0 and final_alpha_cumprod = alphas_cumprod[0])
        same_tables = self.scheduler_bwd.timesteps.tolist() == self._loop.t_bwd.tolist() and not cfg.set_alpha_to_one
        return same_tables and self._unwatched()

    def diffusion_forward(self, latent, context, guidance_scale_fwd: Optional[float] = None) -> Dict[str, Any]:
        """(:71-104) -> latents: the corrected latent of every step in ascending t, then the noisiest sampled latent; noise_preds, etas,
        variance_noises per step, the first (t smallest) noise map zeroed"""
        scale = guidance_scale_fwd or self.guidance_scale_fwd
        noise = self._draw(latent)
        S = self.num_inference_steps
        if self._fast() and latent.shape[0] == 1 and context.shape[0] == 2:
            res = self._loop.invert(latent.float(), context[None].float(), noise, scale)
            by_t = lambda v: [v[S - 1 - i] for i in range(S)]                   # the loop's tensors follow xts: index 0 = the largest t
            latents, noise_preds, zs = by_t(res["latents"]), by_t(res["noise_preds"]), by_t(res["zs"])
            latents.append(res["xts"][0])
        else:
            xts = self.scheduler_fwd.sample_latents(latent, noise=noise)
            latents, noise_preds, zs = [], [], []
            for t in self.pbar(self.scheduler_fwd.timesteps, desc="forward"):
                x = self.scheduler_fwd.get_sampled_latent_by_t(xts, t)
                x, eps, z = self.predict_step_forward(x, t, context, scale, xts)
                latents.append(x)
                noise_preds.append(eps)
                zs.append(z)
            latents.append(xts[0][None])
            zs[0] = torch.zeros_like(zs[0])
        etas = [self.scheduler_fwd.get_eta_by_t(t) for t in self.scheduler_fwd.timesteps]
        return {"latents": latents, "noise_preds": noise_preds, "etas": etas, "variance_noises": zs}

    # ------------------------------------------------------------------ backward pass
    def get_bwd_skip(self) -> int:
        """(:120-126) how many denoising steps are skipped"""
        return int(self.skip_steps * len(self.scheduler_bwd.timesteps))

    def skip_inv_result(self, inv_result: Dict[str, Any]) -> Dict[str, Any]:
        """(:106-118) cut the skipped steps off the inversion result; every other key passes.  A skip of 0 cuts nothing (the reference's `[:-0]`
        would cut everything)"""
        skip = self.get_bwd_skip()
        cut = {k: list(inv_result[k])[:len(inv_result[k]) - skip] for k in ("latents", "noise_preds", "variance_noises", "etas")}
        return {**inv_result, **cut}

    def sample(self, inv_result: Dict[str, Any], prompt: Optional[Union[str, List[str]]] = None,
               context: Optional[Union[torch.Tensor, List[torch.Tensor]]] = None) -> Dict[str, Any]:
        if inv_result is not None and self.skip_steps is not None:
            inv_result = self.skip_inv_result(inv_result)
        return super().sample(inv_result, prompt=prompt, context=context)

    def _scales(self, rows: int) -> List[float]:
        """(:154-159) [source, target] rows run under [guidance_scale_fwd, guidance_scale_bwd]; a single row under guidance_scale_bwd"""
        if rows == 2:
            return [float(self.guidance_scale_fwd), float(self.guidance_scale_bwd)]
        if rows != 1:
            raise AssertionError(f"the backward pass takes one latent or a [source, target] pair, got {rows}")
        return [float(self.guidance_scale_bwd)]

    def predict_step_backward(self, latent, t, context, eta: float, variance_noise: torch.Tensor, guidance_scale_bwd: Optional[float] = None):
        """(:135-166) one hooked step: both halves of every row run, each prompt row is guided under its own scale, then DDIMScheduler.step with
        the noise map as variance noise"""
        latent = self.controller.begin_step(latent=latent)
        n = latent.shape[0]
        scales = self._scales(n)
        eps = self.unet(latent.repeat(2, 1, 1, 1), t, encoder_hidden_states=context)["sample"]
        noise_pred = torch.cat([self._cfg(torch.cat([eps[r:r + 1], eps[n + r:n + r + 1]]), scales[r]) for r in range(n)])
        latent = self.step_backward(noise_pred, t, latent, eta=eta, variance_noise=variance_noise).prev_sample
        latent = self.controller.end_step(latent=latent, noise_pred=noise_pred, t=t)
        return latent, noise_pred

    def diffusion_backward(self, latent, context, inv_result):
        """(:168-177) the steps behind the skip, noisiest first, each with the noise map of its timestep"""
        etas = list(reversed(inv_result["etas"]))
        zs = list(reversed(inv_result["variance_noises"]))
        timesteps = self.scheduler_bwd.timesteps[self.get_bwd_skip():]
        assert len(zs) == len(timesteps), f"{len(zs)} noise maps for {len(timesteps)} backward steps"
        if self._fast() and context.shape[0] == 2 * latent.shape[0]:
            return self._loop.backward(latent, context, zs, self._scales(latent.shape[0])).to(latent.dtype)
        for i, t in enumerate(self.pbar(timesteps, desc="backward")):
            latent, _ = self.predict_step_backward(latent, t, context, etas[i], zs[i], self.guidance_scale_bwd)
        return latent
