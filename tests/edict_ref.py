"""Restatement of EDICT (coupled-pair inversion; reference modules/inversion/edict_inversion.py) in numpy: the reference of the native
`edict` inverter (csrc/step_kernels.hip etainv_edict_*, etainv.pipeline.EdictLoop, modules/inversion/edict_inversion.py).
tests/test_edict_ref.py pins it, without a GPU, against goldens recorded from the reference implementation (tests/golden/edict_steps.npz,
e2e_edict.npz).

Precision: the step coefficients are host scalars that the reference computes with fp32 tensor arithmetic on the fp32 alphas_cumprod table
(edict_inversion.py:82-111,157-171,207-221); `coefficients` repeats that arithmetic in fp32, operation by operation (b is a difference of two
terms of similar size, so a float64 b would sit up to 1e-6 away from what the reference multiplies with).  The square roots are taken by
torch like there: its fp32 sqrt is not always the correctly rounded one (sqrt(1 - abar_520) comes out one ulp below numpy's), and one ulp of
a 0.87 term is 1.06e-6 of b = 0.056 at S = 50.  Everything that touches a latent -- the coupled update, the mix, the loops -- is float64."""
import numpy as np

NUM_TRAIN = 1000


def alphas_cumprod32():
    """fp32 table of the SD1.x scheduler (scaled_linear 0.00085..0.012), as torch builds it"""
    import torch
    betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, NUM_TRAIN, dtype=torch.float32) ** 2
    return torch.cumprod(1.0 - betas, dim=0).numpy()


def timesteps(S, init_image_strength=1.0):
    """(forward, backward) timesteps actually run: leading spacing, the t_limit noisiest ones cut off (edict_inversion.py:258,422-428)"""
    t_bwd = (np.arange(S) * (NUM_TRAIN // S))[::-1].astype(np.int64)
    t_limit = S - int(S * init_image_strength)
    return t_bwd[::-1][:S - t_limit].copy(), t_bwd[t_limit:].copy()


def alpha_at(ac32, t):
    """get_alpha_and_beta (:82-111) for an integer timestep (table lookup) or the float `t - 1000 / S` (negative: final_alpha_cumprod =
    alphas_cumprod[0]; else `low * rem + high * (1 - rem)`: the weights are the reverse of a linear interpolation, kept as written)"""
    if isinstance(t, (int, np.integer)):
        return np.float32(ac32[int(t)])
    t = np.float32(t)
    if t < 0:
        return np.float32(ac32[0])
    low, high = int(np.floor(t)), int(np.ceil(t))
    rem = np.float32(t - np.float32(low))
    return np.float32(np.float32(ac32[low] * rem) + np.float32(ac32[high] * np.float32(np.float32(1) - rem)))


def _sqrt32(v):
    import torch
    return np.float32(torch.sqrt(torch.tensor(float(v), dtype=torch.float32)).item())


def coefficients(ac32, t, S, inverse):
    """(a, b, abar_t, abar_prev) of x' = a x + b eps at integer timestep t: EdictScheduler.step (inverse False, :157-173, eta = 0) or
    EdictSchedulerInverse.step (:207-222); fp32 like the reference"""
    f = np.float32
    prev = f(f(int(t)) - f(NUM_TRAIN / S))               # the long timestep minus a Python float: an fp32 tensor
    a_t, a_p = alpha_at(ac32, int(t)), alpha_at(ac32, prev)
    q = _sqrt32(f(a_t / a_p))
    if inverse:
        a, b = q, f(_sqrt32(f(f(1) - a_t)) - f(q * _sqrt32(f(f(1) - a_p))))
    else:
        a = f(f(1) / q)
        b = f(_sqrt32(f(f(1) - a_p)) - f(a * _sqrt32(f(f(1) - a_t))))
    return a, b, a_t, a_p


def order(i, S, is_fwd, leapfrog_steps=True):
    """iter_latent_pair (:288-315): which latent of the pair is updated first / second at step index i (of the truncated timestep list);
    S = the FULL number of scheduler timesteps, whatever init_image_strength cut off"""
    if is_fwd:
        off = (S - (i + 1) + 1) % 2 if leapfrog_steps else 1
    else:
        off = i % 2
    return [off % 2, (1 + off) % 2]


def mix(pair, p, inverse):
    """sync_latent_pair (:317-338)"""
    x, y = pair
    if inverse:
        y = (y - (1 - p) * x) / p
        x = (x - (1 - p) * y) / p
    else:
        x = p * x + (1 - p) * y
        y = (1 - p) * x + p * y
    return [x, y]


class EdictRef:
    """invert / sample over a callable unet(x (n,4,L,L) float64, t int, ctx (n,77,768)) -> eps (n,4,L,L)."""

    def __init__(self, unet, S, guidance_scale_fwd=3.0, guidance_scale_bwd=3.0, mix_weight=0.93, leapfrog_steps=True, init_image_strength=1.0):
        self.unet, self.S, self.g_fwd, self.g_bwd = unet, S, guidance_scale_fwd, guidance_scale_bwd
        self.p, self.leapfrog = mix_weight, leapfrog_steps
        self.ac = alphas_cumprod32()
        self.t_fwd, self.t_bwd = timesteps(S, init_image_strength)

    def eps(self, x, t, context, g):
        """predict_noise (diffusion_inversion.py:249-286): context rows [uncond x n, cond x n] over the n latents; scale 0 / 1 run one half"""
        n = context.shape[0] // 2
        if g == 0:
            return self.unet(x, t, context[:n])
        if g == 1:
            return self.unet(x, t, context[n:])
        u, c = np.split(self.unet(np.concatenate([x, x]), t, context), 2)
        return u + g * (c - u)

    def step_forward(self, pair, i, context, g=None):
        g = g or self.g_fwd
        t = int(self.t_fwd[i])
        a, b, _, _ = coefficients(self.ac, t, self.S, True)
        pair = mix(pair, self.p, True)
        for k in order(i, self.S, True, self.leapfrog):
            pair[k] = float(a) * pair[k] + float(b) * self.eps(pair[1 - k], t, context, g)
        return pair

    def step_backward(self, pair, i, context, g=None, begin_step=None, end_step=None):
        """begin_step(k) / end_step(k, latent) -> latent: the controller of pair member k around its half-step (EdictController, controller.py:71-110)"""
        g = g or self.g_bwd
        t = int(self.t_bwd[i])
        a, b, _, _ = coefficients(self.ac, t, self.S, False)
        pair = list(pair)
        for k in order(i, self.S, False):
            if begin_step is not None:
                begin_step(k)
            pair[k] = float(a) * pair[k] + float(b) * self.eps(pair[1 - k], t, context, g)
            if end_step is not None:
                pair[k] = end_step(k, pair[k])
        return mix(pair, self.p, False)

    def invert(self, z0, context, g=None):
        """-> trajectory [pair_0 .. pair_S'] (pair_0 = two copies of z0)"""
        z0 = np.asarray(z0, dtype=np.float64)
        traj = [[z0.copy(), z0.copy()]]
        for i in range(len(self.t_fwd)):
            traj.append(self.step_forward(list(traj[-1]), i, context, g))
        return traj

    def sample(self, pair, contexts, begin_step=None, end_step=None):
        """contexts: list of (2,77,768) [uncond, cond]; the pair is repeated once per context (rows [src, tgt]) -> final pair"""
        n = len(contexts)
        context = np.stack(contexts, 1).reshape(2 * n, *contexts[0].shape[1:])
        pair = [np.concatenate([np.asarray(v, dtype=np.float64)] * n) for v in pair]
        for i in range(len(self.t_bwd)):
            pair = self.step_backward(pair, i, context, begin_step=begin_step, end_step=end_step)
        return pair


def torch_unet(unet):
    """wrap an oracle UNet (torch module: unet(x, t, encoder_hidden_states=ctx)["sample"]) as the callable EdictRef takes"""
    import torch
    dt = next(unet.parameters()).dtype

    def call(x, t, ctx):
        with torch.no_grad():
            out = unet(torch.from_numpy(np.ascontiguousarray(x)).to(dt), torch.tensor(int(t)), encoder_hidden_states=torch.from_numpy(np.ascontiguousarray(ctx)).to(dt))["sample"]
        return out.double().numpy()
    return call


def roundtrip_error(pair, z0):
    """relative L2 distance of a reconstruction from z0; for a pair, the worse of its two members"""
    z0 = np.asarray(z0, dtype=np.float64)
    return max(float(np.linalg.norm(np.asarray(v, dtype=np.float64) - z0) / np.linalg.norm(z0)) for v in pair)


# ---- the SD-width case of tests/golden/edict_sd.npz (make_edict_golden.py --oracle) and tests/test_edict_gpu.py: inputs drawn from seeds
SD_L, SD_S = 16, 3


def sd_case_inputs():
    """z0 (1,4,L,L), ctx_src, ctx_tgt (2,77,768) [uncond, cond] with a shared uncond row, float64 values of fp32 draws"""
    import torch
    g = torch.Generator().manual_seed(31)
    z0 = 0.8 * torch.randn(1, 4, SD_L, SD_L, generator=g)
    unc, cs, ct = (torch.randn(77, 768, generator=g) for _ in range(3))
    ct = 0.7 * cs + 0.3 * ct                                   # a target prompt that shares most of the source prompt
    f = lambda v: v.double().numpy()
    return f(z0), f(torch.stack([unc, cs])), f(torch.stack([unc, ct]))
