"""EDICT (exact diffusion inversion via coupled transformations) on the native engine.  Plugin surface of the reference's
modules/inversion/edict_inversion.py:17-447: `EdictScheduler` / `EdictSchedulerInverse` wrap the native DDIM scheduler, `EdictInversion`
keeps a pair of latents (a two-element list) that is un-mixed before every inversion step and mixed after every denoising step, each member
updated from a UNet call on the other.  `invert` + `sample` without an attention controller run the batched device loop
`etainv.pipeline.EdictLoop`; the per-step methods call the same C-ABI kernels (etainv_edict_couple / etainv_edict_mix) one step at a time."""
import contextlib
from typing import Iterator, List, Optional, Tuple

import torch

from etainv import _capi
from etainv.pipeline import EdictLoop, edict_alpha, edict_coefficients
from ..editing.controller import ControllerBase, ControllerEmpty, EdictController
from ..schedulers import DDIMScheduler
from .diffusion_inversion import DiffusionInversion


class EdictSchedulerBase:
    """wrapper of the DDIM scheduler whose `step` is the EDICT update x' = a x + b eps (reference :17-134)"""
    inverse = False

    def __init__(self, scheduler: Optional[DDIMScheduler] = None) -> None:
        if scheduler is None:
            scheduler = DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", num_train_timesteps=1000,
                                      clip_sample=False, set_alpha_to_one=False)
        self.scheduler = scheduler

    def set_timesteps(self, num_inference_steps: int) -> None:
        self.scheduler.set_timesteps(num_inference_steps)

    @property
    def config(self):
        return self.scheduler.config

    @property
    def timesteps(self) -> torch.Tensor:
        return self.scheduler.timesteps

    @property
    def num_inference_steps(self) -> int:
        return self.scheduler.num_inference_steps

    @property
    def alphas_cumprod(self) -> torch.Tensor:
        return self.scheduler.alphas_cumprod

    def get_alpha_and_beta(self, t: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        alpha = edict_alpha(self.scheduler.alphas_cumprod, self.scheduler.final_alpha_cumprod, t)
        return alpha, 1 - alpha

    def coefficients(self, timestep) -> Tuple[float, float]:
        return edict_coefficients(self.scheduler.alphas_cumprod, self.scheduler.final_alpha_cumprod, int(timestep), self.num_inference_steps,
                                  self.inverse)

    def step(self, model_output, timestep, sample, eta: float = 0, variance_noise=None):
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        if int(timestep) > int(self.timesteps.max()):
            raise NotImplementedError(f"timestep {int(timestep)} lies above the scheduler's largest timestep")
        if eta:
            raise NotImplementedError("the EDICT schedulers are built for eta = 0 (the coupled update is exactly invertible only without noise)")
        a, b = self.coefficients(timestep)
        x, eps = sample.contiguous(), model_output.to(sample.dtype).contiguous()
        out = torch.empty_like(x)
        _capi.check(_capi.load().etainv_edict_couple(_capi.ptr(x), None, _capi.ptr(eps), 1.0, a, b, _capi.ptr(out), x.numel(),
                                                     _capi.dtype_code(x.dtype), _capi.stream_ptr()))
        return DDIMScheduler.Output(out)


class EdictScheduler(EdictSchedulerBase):
    """denoising: a = 1 / q, b = sqrt(1 - abar_prev) - sqrt(1 - abar_t) / q, q = sqrt(abar_t / abar_prev) (reference :137-179)"""


class EdictSchedulerInverse(EdictSchedulerBase):
    """inversion: a = q, b = sqrt(1 - abar_t) - q sqrt(1 - abar_prev); its timesteps ascend (reference :182-222)"""
    inverse = True

    @property
    def timesteps(self) -> torch.Tensor:
        return self.scheduler.timesteps.flip(0)


class EdictInversion(DiffusionInversion):
    dft_mix_weight = 0.93
    dft_leapfrog_steps = True
    dft_init_image_strength = 0.8

    def __init__(self, model, scheduler: Optional[str] = None, num_inference_steps: Optional[int] = None,
                 guidance_scale_bwd: Optional[float] = None, guidance_scale_fwd: Optional[float] = None, verbose: bool = False,
                 mix_weight: float = 0.93, leapfrog_steps: bool = True, init_image_strength: float = 1.0, prec=torch.float32) -> None:
        guidance_scale_fwd = guidance_scale_fwd or 3.0
        guidance_scale_bwd = guidance_scale_bwd or 3.0
        if not 0.0 < float(mix_weight) <= 1.0:
            raise ValueError(f"mix_weight must be in (0, 1], got {mix_weight}")
        self.mix_weight, self.leapfrog_steps, self.init_image_strength = mix_weight, leapfrog_steps, init_image_strength
        self.t_limit = (num_inference_steps or 50) - int((num_inference_steps or 50) * init_image_strength)
        super().__init__(model, scheduler, num_inference_steps, guidance_scale_bwd, guidance_scale_fwd, verbose)
        # timestep -> step index over the truncated lists (the base class maps the full ones)
        self.bwd_t_to_i = {t.item(): i for i, t in enumerate(self.get_timesteps_backward())}
        self.fwd_t_to_i = {t.item(): i for i, t in enumerate(self.get_timesteps_forward())}
        self.L = model.engine.L
        self._loop = EdictLoop(model.engine, S=self.num_inference_steps, guidance_scale_fwd=self.guidance_scale_fwd,
                               guidance_scale_bwd=self.guidance_scale_bwd, mix_weight=mix_weight, leapfrog_steps=leapfrog_steps,
                               init_image_strength=init_image_strength)

    @contextlib.contextmanager
    def use_controller(self, controller: Optional[ControllerBase]) -> Iterator[None]:
        self.controller = EdictController(controller if controller is not None else ControllerEmpty())   # one copy per pair member
        self.controller.begin()
        try:
            yield
        finally:
            self.controller.end()
            self.controller = EdictController(ControllerEmpty())

    def create_schedulers(self, model, scheduler, num_inference_steps, scheduler_inv_kwargs=None):
        if not self._plain_ddim(scheduler, dict_type=True, unnamed=False):
            # (the reference throws the inverse scheduler away and wraps whatever backward scheduler it got as if it were DDIM, :279-286)
            raise NotImplementedError(f"edict steps both passes with its own DDIM-form update; scheduler '{scheduler}' is not built for it (use 'ddim')")
        sched, bwd, _ = super().create_schedulers(model, scheduler, num_inference_steps, scheduler_inv_kwargs)
        return sched, EdictScheduler(bwd), EdictSchedulerInverse(bwd)

    # ------------------------------------------------------------------ the pair
    def iter_latent_pair(self, i: int, latent_pair: List[torch.Tensor], is_fwd: bool = False):
        """(index, (that latent, the other latent)) in EDICT's order for step i; the second item sees the first one's update (reference :288-315)"""
        for latent_i in range(2):
            if is_fwd:
                if self.leapfrog_steps:
                    orig_i = len(self.scheduler_fwd.timesteps) - (i + 1)          # the step index counted from the other end
                    latent_i = (latent_i + (orig_i + 1) % 2) % 2
                else:
                    latent_i = (latent_i + 1) % 2
            else:
                latent_i = (latent_i + i % 2) % 2
            latent_j = (latent_i + 1) % 2
            yield latent_i, (latent_pair[latent_i], latent_pair[latent_j])

    def sync_latent_pair(self, latent_pair: List[torch.Tensor], is_fwd: bool) -> List[torch.Tensor]:
        """mix (denoising) / un-mix (inversion) the pair, on copies (reference :317-338)"""
        x, y = (v.clone().contiguous() for v in latent_pair)
        _capi.check(_capi.load().etainv_edict_mix(_capi.ptr(x), _capi.ptr(y), float(self.mix_weight), int(bool(is_fwd)), x.numel(),
                                                  _capi.dtype_code(x.dtype), _capi.stream_ptr()))
        return [x, y]

    def predict_noise(self, latent, t, context, guidance_scale, is_fwd: bool = False, latent_idx: Optional[int] = None, **kwargs):
        return super().predict_noise(latent, t, context, guidance_scale, is_fwd, **kwargs)

    def predict_step_forward_single(self, latent_idx, latent_base, latent_model_input, t, context, guidance_scale):
        noise_pred = self.predict_noise(latent_model_input, t, context, guidance_scale, is_fwd=True, latent_idx=latent_idx)
        return self.step_forward(noise_pred, t, latent_base).prev_sample.to(latent_base.dtype)

    def predict_step_backward_single(self, latent_idx, latent_base, latent_model_input, t, context, guidance_scale):
        self.controller.begin_step(latent_idx, latent_base, latent_model_input)
        noise_pred = self.predict_noise(latent_model_input, t, context, guidance_scale, is_fwd=False, latent_idx=latent_idx)
        new_latent = self.step_backward(noise_pred, t, latent_base).prev_sample.to(latent_base.dtype)
        return self.controller.end_step(latent=new_latent, noise_pred=noise_pred, t=t)

    def predict_step_forward(self, latent, t, context, guidance_scale_fwd=None):
        guidance_scale_fwd = guidance_scale_fwd or self.guidance_scale_fwd
        i = self.fwd_t_to_i[t.item()]
        latent_pair = self.sync_latent_pair(latent, is_fwd=True)
        for latent_idx, (latent_base, latent_model_input) in self.iter_latent_pair(i, latent_pair, is_fwd=True):
            latent_pair[latent_idx] = self.predict_step_forward_single(latent_idx, latent_base, latent_model_input, t, context, guidance_scale_fwd)
        return latent_pair, None

    def predict_step_backward(self, latent, t, context, guidance_scale_bwd=None):
        guidance_scale_bwd = guidance_scale_bwd or self.guidance_scale_bwd
        i = self.bwd_t_to_i[t.item()]
        latent_pair = list(latent)
        for latent_idx, (latent_base, latent_model_input) in self.iter_latent_pair(i, latent_pair, is_fwd=False):
            latent_pair[latent_idx] = self.predict_step_backward_single(latent_idx, latent_base, latent_model_input, t, context, guidance_scale_bwd)
        return self.sync_latent_pair(latent_pair, is_fwd=False), None

    def get_timesteps_forward(self) -> torch.Tensor:
        ts = super().get_timesteps_forward()
        return ts[:-self.t_limit] if self.t_limit != 0 else ts

    def get_timesteps_backward(self) -> torch.Tensor:
        ts = super().get_timesteps_backward()
        return ts[self.t_limit:] if self.t_limit != 0 else ts

    def encode(self, image) -> List[torch.Tensor]:
        latent = super().encode(image)
        return [latent.clone(), latent.clone()]

    def decode(self, latent: List[torch.Tensor]) -> torch.Tensor:
        return super().decode(torch.cat(latent))

    def cat_latent(self, latents: List[List[torch.Tensor]]) -> List[torch.Tensor]:
        assert len(latents[0]) == 2
        return [torch.cat([pair[m] for pair in latents]) for m in range(2)]

    # ------------------------------------------------------------------ loops
    def _fast(self) -> bool:
        """the batched device loop serves the passes that no controller watches (force_per_step, an attribute, keeps the per-step path)"""
        return self._unwatched(self.controller.controllers)              # (one copy of the controller per pair member)

    def diffusion_forward(self, latent, context, guidance_scale_fwd=None):
        scale = guidance_scale_fwd or self.guidance_scale_fwd
        if self._fast() and context.shape[0] == 2 and latent[0].shape[0] == 1 and torch.equal(latent[0], latent[1]):
            res = self._loop.invert(latent[0].float().contiguous(), context[None].float(), scale)
            lat = res["latents"]
            pairs = [[lat[j, 0], lat[j, 1]] for j in range(lat.shape[0])]
            return {"latents": pairs, "noise_preds": None, "zT_inv": pairs[-1], "_native": res}
        trajectory = [latent]
        pair = [v.clone().detach().float() for v in latent]
        for t in self.pbar(self.get_timesteps_forward(), desc="forward"):
            pair, _ = self.predict_step_forward(pair, t, context, scale)
            trajectory.append(pair)
        return {"latents": trajectory, "noise_preds": [None] * (len(trajectory) - 1), "zT_inv": trajectory[-1]}

    def diffusion_backward(self, latent, context, inv_result):
        n = latent[0].shape[0]
        if self._fast() and context.shape[0] == 2 * n and "_native" in inv_result:
            ctx = context.reshape(2, n, *context.shape[1:])
            pair = self._loop.sample(inv_result["_native"], [ctx[:, m][None] for m in range(n)])
            return [pair[0], pair[1]]
        for t in self.pbar(self.get_timesteps_backward(), desc="backward"):
            latent, _ = self.predict_step_backward(latent, t, context)
        return latent

    def invert(self, image, prompt=None, context=None, guidance_scale_fwd=None, **kwargs):
        context = context if context is not None else self.create_context(prompt)
        latent = [v.float() for v in self.encode(image)]
        res = self.diffusion_forward(latent, context, guidance_scale_fwd=guidance_scale_fwd)
        res["context"] = context
        return {**kwargs, **res}
