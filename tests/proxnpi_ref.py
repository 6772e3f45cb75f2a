"""Restatement of negative-prompt inversion and proximal negative-prompt inversion (reference modules/inversion/negative_prompt_inversion.py,
proximal_negative_prompt_inversion.py): the reference of the native `npi` / `proxnpi` inverters (csrc/proximal.hip etainv_prox_guidance,
etainv.pipeline.ProximalGuidance, modules/inversion/negative_prompt_inversion.py, proximal_negative_prompt_inversion.py).
tests/test_proxnpi_ref.py pins it, without a GPU, against fixtures recorded from the reference implementation (tests/golden/proxnpi_guidance.npz,
e2e_npi.npz).

The guidance takes its threshold from SORTED ORDER STATISTICS at the rank split of torch.quantile -- no call of torch.quantile -- in float64 or
in float32 (`dtype`): in float32 every operation rounds where the reference's fp32 run and the kernel round."""
import numpy as np

from tests.regdiff_ref import NUM_TRAIN, alphas_cumprod, ddim_inverse_step

QUANTILES = (0.7, 0.3, 1.0, 0, -0.25)
GUIDANCE_SHAPES = ((1, 4, 8, 8), (2, 4, 8, 8), (2, 4, 20, 20), (3, 4, 12, 12))
GUIDANCE_INPUTS = ("white", "zero_row", "eighths")


def rank_split(n, q, dtype=np.float32):
    """(k, w) of torch.quantile over n values of `dtype`: rank = dtype(q) * (n - 1) in that type, k = floor(rank), w = rank - k"""
    rank = dtype(q) * dtype(n - 1)
    k = min(int(np.floor(rank)), n - 1)
    return k, dtype(rank - dtype(k))


def lerp(a, b, w):
    """torch.lerp's rule in the type of its arguments"""
    diff = b - a
    return a + w * diff if w < 0.5 else b - diff * (type(w)(1) - w)


def threshold(d, quantile, dtype=np.float64):
    """the threshold of proximal_guidance (:84-87, :101-107) over the whole array d, and the two order statistics it lies between"""
    if quantile <= 0:
        thr = dtype(0.0 - quantile)
        return thr, thr, thr
    mags = np.sort(np.abs(np.asarray(d, dtype=dtype)).ravel())
    k, w = rank_split(mags.size, quantile, dtype)
    lo, hi = mags[k], mags[min(k + 1, mags.size - 1)]
    return lerp(lo, hi, w), lo, hi


def shrink(d, thr, prox):
    """:88-90 (l1) and :108 (l0), in d's type"""
    out = d - np.clip(d, -thr, thr)
    if prox == "l1":
        out = np.where(out > 0, out - thr, out)
        out = np.where(out < 0, out + thr, out)
    elif prox != "l0":
        raise NotImplementedError(prox)
    return out


def guidance(eps_u, eps_c, g, prox="l0", quantile=0.7, dtype=np.float64):
    """proximal_guidance (:61-128) -> (noise, threshold or None)"""
    u, c = np.asarray(eps_u, dtype=dtype), np.asarray(eps_c, dtype=dtype)
    d = c - u
    if prox is None:
        return u + dtype(g) * d, None
    thr = threshold(d, quantile, dtype)[0]
    return u + dtype(g) * shrink(d, thr, prox), thr


def guidance_inputs(shape, kind, seed):
    """(eps_u, eps_c) fp32 draws from a seeded CPU generator.  white: independent normal draws; zero_row: the first row's d is exactly zero
    (eps_c = eps_u there: the source pair of an edit); eighths: eps_u and eps_c in multiples of 1/8, so d is too and ties are everywhere"""
    import torch
    gen = torch.Generator().manual_seed(seed)
    u, c = torch.randn(shape, generator=gen), torch.randn(shape, generator=gen)
    if kind == "zero_row":
        c[0] = u[0]
    elif kind == "eighths":
        u, c = torch.round(u * 8) / 8, torch.round(c * 8) / 8
    elif kind != "white":
        raise ValueError(kind)
    return u.numpy(), c.numpy()


def guidance_seed(shape, kind):
    return 7000 + 100 * GUIDANCE_SHAPES.index(tuple(shape)) + GUIDANCE_INPUTS.index(kind)


class NpiRef:
    """invert / sample over a callable unet(x (n,4,L,L) float64, t int, ctx (n,77,768)) -> eps (n,4,L,L).
    invert: the base class's DDIM inversion at guidance 1 (the cond half alone, diffusion_inversion.py:277-278).
    sample: negative_prompt_inversion.py:17-23 -- every unconditional row of the context is the SOURCE prompt's conditional embedding -- with
    plain CFG (prox None) or proximal guidance over all rows of the call (prox "l0" / "l1")."""

    def __init__(self, unet, S, guidance_scale_bwd=7.5, prox=None, quantile=0.7):
        self.unet, self.S, self.g, self.prox, self.quantile = unet, S, guidance_scale_bwd, prox, quantile
        self.ac = alphas_cumprod()
        self.delta = NUM_TRAIN // S
        self.t_fwd = (np.arange(S) * self.delta).astype(np.int64)
        self.t_bwd = self.t_fwd[::-1]

    def _alpha(self, tau):
        return float(self.ac[min(int(tau), NUM_TRAIN - 1)]) if tau >= 0 else float(self.ac[0])

    def invert(self, z0, context):
        """z0 (1,4,L,L), context (2,77,768) [uncond, cond] -> latents (S+1,1,4,L,L)"""
        z = np.asarray(z0, dtype=np.float64)
        lat = [z]
        for t in self.t_fwd:
            eps = self.unet(z, int(t), context[1:2])
            z = ddim_inverse_step(z, eps, self._alpha(int(t) - self.delta), self._alpha(int(t)))
            lat.append(z)
        return np.stack(lat)

    def sample(self, zT, src_context, contexts, guidance_scale=None):
        """contexts: list of (2,77,768) [uncond, cond]; the rows of the call are [uncond x n, cond x n] over n copies of zT.
        -> (latents (n,4,L,L), thresholds (S,), the d of every step (S,n,4,L,L))"""
        g = self.g if guidance_scale is None else guidance_scale
        n = len(contexts)
        cond = np.concatenate([c[1:2] for c in contexts])
        ctx = np.concatenate([np.repeat(src_context[1:2], n, axis=0), cond])
        z = np.concatenate([np.asarray(zT, dtype=np.float64)] * n)
        thrs, ds = [], []
        for t in self.t_bwd:
            u, c = np.split(self.unet(np.concatenate([z, z]), int(t), ctx), 2)
            eps, thr = guidance(u, c, g, self.prox, self.quantile)
            thrs.append(np.nan if thr is None else thr)
            ds.append(c - u)
            z = ddim_inverse_step(z, eps, self._alpha(int(t)), self._alpha(int(t) - self.delta))
        return z, np.array(thrs), np.stack(ds)
