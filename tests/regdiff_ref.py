"""Restatement of regularised DDIM inversion (pix2pix-zero; reference modules/inversion/regularized_diffusion_inversion.py): the reference of
the native `regdiffinv` inverter (csrc/regularize.hip etainv_noise_regularize, etainv.pipeline.NoiseRegularizer / EtaLoop,
modules/inversion/regularized_diffusion_inversion.py).  tests/test_regdiff_ref.py pins it, without a GPU, against fixtures recorded from the
reference implementation (tests/golden/regdiff_reg.npz, e2e_regdiff.npz).

Two forms of the regulariser:
  regularize_closed    float64 numpy, the gradients of both losses written out (no autograd);
  regularize_autograd  torch, the reference's loop over the two losses with autograd, in fp32 or float64 -- in fp32 it is the arithmetic the
                       kernel has (other reduction trees, other contraction), and its distance from float64 is what the kernel tests scale their
                       bound with.
Both read the shifts from a table built once by `shift_table` with the reference's generator call sequence."""
import numpy as np

NUM_TRAIN = 1000
DEFAULTS = dict(lambda_ac=20.0, lambda_kl=20.0, num_reg_steps=5, num_ac_rolls=5)


def level_sizes(L):
    """sizes of the average-pool pyramid of auto_corr_loss (:61-68): the loss is taken at a level, then the level is pooled while it is above 8"""
    sizes = [int(L)]
    while sizes[-1] > 8:
        sizes.append(sizes[-1] // 2)
    return sizes


def shift_table(L, num_reg_steps=5, num_ac_rolls=5, lambda_ac=20.0, generator=None, seed=0):
    """int32 [num_reg_steps * num_ac_rolls][4][levels]: one torch.randint(0, s // 2, ()) per channel, per level (fine to coarse), per
    autocorrelation step, from `generator` or a fresh CPU generator seeded like predict_step_forward (:117) does at every inversion step.
    Nothing is drawn with lambda_ac <= 0 (:99)."""
    import torch
    sizes = level_sizes(L)
    if lambda_ac <= 0:
        return np.zeros((0, 4, len(sizes)), dtype=np.int32)
    g = generator if generator is not None else torch.Generator().manual_seed(seed)
    n = num_reg_steps * num_ac_rolls
    out = np.zeros((n, 4, len(sizes)), dtype=np.int32)
    for a in range(n):
        for c in range(4):
            for k, s in enumerate(sizes):
                out[a, c, k] = torch.randint(0, s // 2, (), generator=g).item()
    return out


def multiscale_field(L, n_img=1, seed=0):
    """the kernel tests' input: white noise + 0.5 x nearest-upsampled white noise at factors 2, 4, 8, 16 + 0.05, fp32 draws from a seeded CPU
    generator -- correlated at every scale, so every pyramid level's term matters (test_regdiff_ref.py checks that)"""
    import torch
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n_img, 4, L, L, generator=g)
    for f in (2, 4, 8, 16):
        m = -(-L // f)
        coarse = torch.randn(n_img, 4, m, m, generator=g)
        x = x + 0.5 * coarse.repeat_interleave(f, 2).repeat_interleave(f, 3)[:, :, :L, :L]
    return x + 0.05


def _pool(n):
    s = n.shape[0] // 2
    return n[:2 * s, :2 * s].reshape(s, 2, s, 2).mean(axis=(1, 3))


def ac_grad(ch, shifts, drop_level=None):
    """gradient of the autocorrelation loss of one channel (L, L) float64: per level m = mean(n roll(n, r)) per axis, its gradient
    2 m / s^2 (roll(n, r) + roll(n, -r)), brought to level 0 by the pool's adjoint (value / 4 over the 2 x 2 block; dropped rows and columns get 0)"""
    pyramid = [ch]
    for _ in range(len(shifts) - 1):
        pyramid.append(_pool(pyramid[-1]))
    total = None
    for k in reversed(range(len(pyramid))):
        n, r = pyramid[k], int(shifts[k])
        s = n.shape[0]
        g = np.zeros_like(n)
        if k != drop_level:
            for axis in (0, 1):
                m = (n * np.roll(n, r, axis)).mean()
                g += 2.0 * m / (s * s) * (np.roll(n, r, axis) + np.roll(n, -r, axis))
        if total is not None:
            c = total.shape[0]
            g[:2 * c, :2 * c] += 0.25 * total.repeat(2, 0).repeat(2, 1)
        total = g
    return total


def kl_grad(e):
    """gradient of var + mu^2 - 1 - log(var + 1e-7) (unbiased var over all N values): an affine map of e"""
    n = e.size
    mu, var = e.mean(), e.var(ddof=1)
    return 2.0 * (e - mu) / (n - 1) * (1.0 - 1.0 / (var + 1e-7)) + 2.0 * mu / n


def regularize_closed(e, shifts=None, lambda_ac=20.0, lambda_kl=20.0, num_reg_steps=5, num_ac_rolls=5, drop_level=None, bump_level=None):
    """regularize_noise_pred (:86-114) for one image e (4, L, L), float64.  drop_level: that pyramid level's loss terms are left out;
    bump_level: that level's shift is offset by one (mod s // 2) -- both only for the input check of the kernel tests."""
    e = np.array(e, dtype=np.float64)
    assert e.ndim == 3 and e.shape[0] == 4 and e.shape[1] == e.shape[2]
    sizes = level_sizes(e.shape[1])
    if shifts is None:
        shifts = shift_table(e.shape[1], num_reg_steps, num_ac_rolls, lambda_ac)
    shifts = np.array(shifts)
    if bump_level is not None and shifts.size:
        shifts[:, :, bump_level] = (shifts[:, :, bump_level] + 1) % (sizes[bump_level] // 2)
    a = 0
    for _ in range(num_reg_steps):
        if lambda_ac > 0:
            for _ in range(num_ac_rolls):
                grad = np.stack([ac_grad(e[c], shifts[a, c], drop_level) for c in range(4)])
                e = e - lambda_ac * (grad / num_ac_rolls)
                a += 1
        if lambda_kl > 0:
            e = e - lambda_kl * kl_grad(e)
    return e


def auto_corr_loss_torch(x, shifts):
    """auto_corr_loss (:42-69) of one image (4, L, L) with the shifts of one autocorrelation step [4][levels]"""
    import torch
    import torch.nn.functional as F
    loss = 0.0
    for c in range(x.shape[0]):
        noise = x[c][None, None]
        k = 0
        while True:
            r = int(shifts[c][k])
            loss = loss + (noise * torch.roll(noise, shifts=r, dims=2)).mean() ** 2
            loss = loss + (noise * torch.roll(noise, shifts=r, dims=3)).mean() ** 2
            if noise.shape[2] <= 8:
                break
            noise = F.avg_pool2d(noise, kernel_size=2)
            k += 1
    return loss


def kl_divergence_torch(x):
    import torch
    mu, var = x.mean(), x.var()
    return var + mu ** 2 - 1 - torch.log(var + 1e-7)


def regularize_autograd(e, shifts=None, lambda_ac=20.0, lambda_kl=20.0, num_reg_steps=5, num_ac_rolls=5, dtype=None):
    """the reference's loop, with autograd, on a torch tensor (4, L, L) in `dtype` (default: the tensor's own)"""
    import torch
    e = torch.as_tensor(e)
    e = e.detach().clone().to(dtype or e.dtype)
    if shifts is None:
        shifts = shift_table(e.shape[1], num_reg_steps, num_ac_rolls, lambda_ac)
    a = 0
    with torch.enable_grad():
        for _ in range(num_reg_steps):
            if lambda_ac > 0:
                for _ in range(num_ac_rolls):
                    v = e.detach().clone().requires_grad_(True)
                    auto_corr_loss_torch(v, shifts[a]).backward()
                    e = e - lambda_ac * (v.grad.detach() / num_ac_rolls)
                    a += 1
            if lambda_kl > 0:
                v = e.detach().clone().requires_grad_(True)
                kl_divergence_torch(v).backward()
                e = e - lambda_kl * v.grad.detach()
            e = e.detach()
    return e


KERNEL_SIZES = (8, 16, 20, 44, 64, 96)     # one level; two; an odd level (20, 10, 5); odd in the middle (44, 22, 11, 5); the LDS limit; five levels, level 0 in L2
KERNEL_BOUND_FACTOR = 8.0
_cases = {}


def kernel_case(L, **params):
    """the input of the kernel tests at size L and what they compare with, computed once: x (3,4,L,L) fp32, the shift table, the float64
    closed form per image, and the bound per image = KERNEL_BOUND_FACTOR x max |fp32 autograd restatement - float64| on that image"""
    import torch
    key = (L, tuple(sorted(params.items())))
    if key not in _cases:
        kw = {**DEFAULTS, **params}
        x = multiscale_field(L, 3, seed=100 + L)
        shifts = shift_table(L, kw["num_reg_steps"], kw["num_ac_rolls"], kw["lambda_ac"])
        ref = np.stack([regularize_closed(v.double().numpy(), shifts, **kw) for v in x])
        dev32 = np.array([np.abs(regularize_autograd(v, shifts, dtype=torch.float32, **kw).double().numpy() - r).max() for v, r in zip(x, ref)])
        _cases[key] = dict(x=x, shifts=shifts, ref=ref, dev32=dev32, bound=KERNEL_BOUND_FACTOR * dev32, params=kw)
    return _cases[key]


def alphas_cumprod():
    import torch
    betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, NUM_TRAIN, dtype=torch.float32) ** 2
    return torch.cumprod(1.0 - betas, dim=0).numpy().astype(np.float64)


def ddim_inverse_step(x, eps, a_from, a_to):
    """DDIMInverseScheduler.ddim_step (scheduling_ddim_inverse.py:71-100)"""
    x0 = (x - np.sqrt(1.0 - a_from) * eps) / np.sqrt(a_from)
    return np.sqrt(a_to) * x0 + np.sqrt(1.0 - a_to) * eps


def guidance(t):
    """predict_step_forward (:120): the forward guidance is linspace(2, 1, 1000)[t], whatever scale was passed"""
    return float(np.linspace(2, 1, NUM_TRAIN)[int(t)])


class RegDiffRef:
    """invert over a callable unet(x (n,4,L,L) float64, t int, ctx (n,77,768)) -> eps (n,4,L,L): per step the guided noise at
    linspace(2, 1, 1000)[t], regularised with the step-independent shift table, then the "sameshift" DDIM inverse step of the loop."""

    def __init__(self, unet, S, regularize=True, **params):
        self.unet, self.S, self.regularize = unet, S, regularize
        self.params = {**DEFAULTS, **params}
        self.ac = alphas_cumprod()
        self.delta = NUM_TRAIN // S
        self.t_fwd = (np.arange(S) * self.delta).astype(np.int64)

    def _alpha(self, tau):
        return float(self.ac[min(int(tau), NUM_TRAIN - 1)]) if tau >= 0 else float(self.ac[0])

    def invert(self, z0, context):
        """z0 (1,4,L,L), context (2,77,768) [uncond, cond] -> (latents (S+1,1,4,L,L), regularised noises (S,1,4,L,L))"""
        z = np.asarray(z0, dtype=np.float64)
        shifts = shift_table(z.shape[-1], self.params["num_reg_steps"], self.params["num_ac_rolls"], self.params["lambda_ac"])
        lat, noises = [z], []
        for t in self.t_fwd:
            u, c = np.split(self.unet(np.concatenate([z, z]), int(t), context), 2)
            eps = u + guidance(t) * (c - u)
            if self.regularize:
                eps = np.stack([regularize_closed(e, shifts, **self.params) for e in eps])
            z = ddim_inverse_step(z, eps, self._alpha(int(t) - self.delta), self._alpha(int(t)))
            lat.append(z)
            noises.append(eps)
        return np.stack(lat), np.stack(noises)
