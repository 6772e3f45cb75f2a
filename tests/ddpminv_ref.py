"""Restatement of edit-friendly DDPM inversion (reference modules/inverse_schedulers/ddpm_inverse_scheduler.py, modules/inversion/ddpm_inversion.py):
the reference of the native `ddpminv` / `cyclediff` inverters (csrc/ddpm.hip, modules/inverse_schedulers/ddpm_inverse_scheduler.py,
modules/inversion/ddpm_inversion.py, etainv.pipeline.DdpmLoop).  tests/test_ddpminv_ref.py pins it, without a GPU, against fixtures recorded
from the reference implementation (tests/golden/ddpm_inverse.npz, e2e_ddpminv.npz).

Everything is numpy in `dtype` (float64 by default; float32 rounds after every operation, as the reference's fp32 run and the kernels do).  The
caller supplies the noise: [S][n][4][L][L] in the reference's draw order, ascending t.

Two places where this restatement, like the native code, does not follow the reference to the letter:
  sigma == 0   at t = 0 (steps_offset 0) the reference divides by zero; here z = 0 and the corrected latent is mu.  The reference zeroes that
               noise map afterwards (ddpm_inversion.py:101) and never reads that latent.
  skip == 0    int(skip_steps * S) == 0 makes the reference's `[:-0]` slices empty; here nothing is skipped."""
import numpy as np

from tests.regdiff_ref import NUM_TRAIN, alphas_cumprod

G_FWD, G_BWD, SKIP = 3.5, 9.0, 0.36


# ---- seeded inputs of tests/golden/ddpm_inverse.npz (make_ddpminv_golden.py --reference) and tests/test_ddpm_kernels_gpu.py
KERNEL_CASES = tuple((S, L) for S in (1, 5) for L in (8, 16, 24))


def kernel_noise_seed(S, L, img=0):
    return 5200 + 1000 * img + 10 * L + S


def kernel_case(S, L, img=0):
    """(x0 (1,4,L,L), noise (S,1,4,L,L), eps (S,1,4,L,L)) fp32: the noise is what a fresh CPU generator with kernel_noise_seed yields draw by draw,
    i.e. what the reference's sample_latents draws from it; eps stands in for the noise predictions, ascending t"""
    import torch
    g = torch.Generator().manual_seed(5100 + 1000 * img + 10 * L + S)
    x0 = 0.8 * torch.randn(1, 4, L, L, generator=g)
    eps = torch.randn(S, 1, 4, L, L, generator=g)
    gn = torch.Generator().manual_seed(kernel_noise_seed(S, L, img))
    noise = torch.stack([torch.randn(1, 4, L, L, generator=gn) for _ in range(S)])
    return x0.numpy(), noise.numpy(), eps.numpy()


def sd_noise(S, shape, seed=41):
    """the forward noise of tests/golden/ddpminv_sd.npz: (S, *shape) float64 values of fp32 draws"""
    import torch
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randn(tuple(shape), generator=g) for _ in range(S)]).double().numpy()


def timesteps(S):
    """the inverse scheduler's timesteps: ascending (ddpm_inverse_scheduler.py:60-63); xts index of timestep i is S - 1 - i"""
    return (np.arange(S) * (NUM_TRAIN // S)).astype(np.int64)


def alpha_prev(ac, t, S):
    """alphas_cumprod[t - 1000 // S], final_alpha_cumprod (= alphas_cumprod[0]: set_alpha_to_one False) below 0"""
    p = int(t) - NUM_TRAIN // S
    return ac[p] if p >= 0 else ac[0]


def variance(ac, t, S):
    """get_variance (:65-84)"""
    a_t, a_p = ac[int(t)], alpha_prev(ac, t, S)
    return (1 - a_p) / (1 - a_t) * (1 - a_t / a_p)


def sample_coefficients(S, markovian, ac=None):
    """(a, b) of x = x' * a + r * b per step in draw order: x' = x0, a = sqrt(abar_t) (:118), or x' = the previous x, a = sqrt(abar_t / abar_prev)
    with abar_prev = 1 below 0 (:121-124)"""
    ac = alphas_cumprod() if ac is None else ac
    out = []
    for t in timesteps(S):
        if markovian:
            p = int(t) - NUM_TRAIN // S
            q = ac[int(t)] / (ac[p] if p >= 0 else 1.0)
            out.append((q ** 0.5, (1 - q) ** 0.5))
        else:
            out.append((ac[int(t)] ** 0.5, (1 - ac[int(t)]) ** 0.5))
    return np.array(out, dtype=np.float64)


def step_coefficients(S, t, ac=None):
    """(sqrt(1 - abar_t), sqrt(abar_t), sqrt(abar_prev), sqrt(1 - abar_prev - var), sqrt(var)) of the inverse step at t (:169-193, eta = 1)"""
    ac = alphas_cumprod() if ac is None else ac
    a_t, a_p, var = ac[int(t)], alpha_prev(ac, t, S), variance(ac, t, S)
    return np.array([(1 - a_t) ** 0.5, a_t ** 0.5, a_p ** 0.5, (1 - a_p - var) ** 0.5, var ** 0.5], dtype=np.float64)


def sample_latents(x0, noise, S, markovian, dtype=np.float64):
    """sample_latents (:86-129): x0 (n,4,L,L), noise (S,n,4,L,L) -> xts (S+1,n,4,L,L), index 0 = the largest t, index S = x0"""
    x0, noise = np.asarray(x0, dtype=dtype), np.asarray(noise, dtype=dtype)
    ab = sample_coefficients(S, markovian).astype(dtype)
    xts = np.empty((S + 1,) + x0.shape, dtype=dtype)
    xts[S] = cur = x0
    for s in range(S):
        cur = (cur if markovian else x0) * ab[s, 0] + noise[s] * ab[s, 1]
        xts[S - 1 - s] = cur
    return xts


def cfg(eps_u, eps_c, g):
    return eps_u + g * (eps_c - eps_u)


def inverse_step(xt, xtm1, eps, coef, dtype=np.float64):
    """step (:156-199) after the noise prediction -> (z, corrected x_{t-1}, mu)"""
    c = np.asarray(coef).astype(dtype)
    xt, xtm1, eps = (np.asarray(v, dtype=dtype) for v in (xt, xtm1, eps))
    x0 = (xt - c[0] * eps) / c[1]
    mu = c[2] * x0 + c[3] * eps
    if c[4] == 0:
        return np.zeros_like(mu), mu, mu
    z = (xtm1 - mu) / c[4]
    return z, mu + c[4] * z, mu


def ddim_eta1_step(x, eps, z, a_t, a_p, var):
    """DDIMScheduler.step(eta = 1, variance_noise = z) as DDPMInversion.predict_step_backward calls it (ddpm_inversion.py:162)"""
    x0 = (x - (1 - a_t) ** 0.5 * eps) / a_t ** 0.5
    std = var ** 0.5
    return a_p ** 0.5 * x0 + (1 - a_p - std ** 2) ** 0.5 * eps + std * z


def bwd_skip(S, skip_steps=SKIP):
    return int(skip_steps * S)


class DdpmInvRef:
    """invert / sample over a callable unet(x (n,4,L,L) float64, t int, ctx (n,77,768)) -> eps (n,4,L,L)."""

    def __init__(self, unet, S, guidance_scale_fwd=G_FWD, guidance_scale_bwd=G_BWD, skip_steps=SKIP, markovian=False):
        self.unet, self.S, self.g_fwd, self.g_bwd, self.skip_steps, self.markovian = unet, S, guidance_scale_fwd, guidance_scale_bwd, skip_steps, markovian
        self.ac = alphas_cumprod()
        self.t_fwd = timesteps(S)
        self.t_bwd = self.t_fwd[::-1]

    def eps(self, x, t, context, g):
        """predict_noise (diffusion_inversion.py:263-286): context [uncond rows, cond rows]; the scales 0 / 1 run one half"""
        n = x.shape[0]
        if isinstance(g, (int, float)) and g in (0, 1):
            return self.unet(x, int(t), context[n:] if g == 1 else context[:n])
        u, c = np.split(self.unet(np.concatenate([x, x]), int(t), context), 2)
        return cfg(u, c, np.asarray(g, dtype=np.float64).reshape(-1, 1, 1, 1) if not isinstance(g, (int, float)) else g)

    def invert(self, z0, context, noise, g=None):
        """diffusion_forward (ddpm_inversion.py:71-104): z0 (1,4,L,L), context (2,77,768) -> dict of xts (S+1,1,4,L,L), latents (S+1,1,4,L,L: the
        corrected latent of every step in ascending t, then xts[0]), noise_preds (S,..), zs (S,..; zs[0] zeroed, :101)"""
        g = self.g_fwd if g is None else g
        xts = sample_latents(z0, noise, self.S, self.markovian)
        lat, eps_seen, zs = [], [], []
        for i, t in enumerate(self.t_fwd):
            idx = self.S - 1 - i
            eps = self.eps(xts[idx], t, context, g)
            z, x, _ = inverse_step(xts[idx], xts[idx + 1], eps, step_coefficients(self.S, t, self.ac))
            lat.append(x)
            eps_seen.append(eps)
            zs.append(z)
        lat.append(xts[0])
        zs[0] = np.zeros_like(zs[0])
        return {"xts": xts, "latents": np.stack(lat), "noise_preds": np.stack(eps_seen), "zs": np.stack(zs)}

    def sample(self, inv, contexts, guidance=None):
        """skip_inv_result + diffusion_backward (:106-177): contexts a list of (2,77,768); rows [uncond x n, cond x n] over n copies of the
        latent; guidance per prompt row: [g_fwd, g_bwd] for two prompts, g_bwd for one (:154-159) -> latents (n,4,L,L)"""
        skip, n = bwd_skip(self.S, self.skip_steps), len(contexts)
        cut = (lambda v: v[:len(v) - skip])                                      # ([:-0] would be empty: a skip of 0 skips nothing)
        lat, zs = cut(inv["latents"]), cut(inv["zs"])
        if guidance is None:
            guidance = [self.g_fwd, self.g_bwd] if n == 2 else [self.g_bwd] * n
        ctx = np.concatenate([np.concatenate([c[0:1] for c in contexts]), np.concatenate([c[1:2] for c in contexts])])
        x = np.concatenate([lat[-1]] * n)
        g = np.asarray(guidance, dtype=np.float64)
        for i, t in enumerate(self.t_bwd[skip:]):
            u, c = np.split(self.unet(np.concatenate([x, x]), int(t), ctx), 2)
            eps = cfg(u, c, g.reshape(-1, 1, 1, 1))
            a_t, a_p = self.ac[int(t)], alpha_prev(self.ac, t, self.S)
            x = ddim_eta1_step(x, eps, zs[len(zs) - 1 - i], a_t, a_p, variance(self.ac, t, self.S))
        return x
