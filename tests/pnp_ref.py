"""Plug-and-play on the oracle's UNet: the reference's three hooks (modules/utils/pnp.py PnPUnetForward with source_latents=None,
modules/utils/pnp_utils.py register_attention_control_efficient / register_conv_control_efficient) restated for n_img images per call, and the
oracle's eta loop run through them.  Pinned against fixtures recorded from the reference's own code by tests/test_pnp_ref.py; the expected values
of the GPU tests (tests/golden/make_pnp_golden.py --oracle) come from here.

Rows of a hooked call: [u_s, u_t, c_t] x n_img.  The reference's `source_batch_size = batch // 3` is n_img."""
import contextlib

import numpy as np
import torch
import torch.nn.functional as F

NEGATIVE_PROMPT = "ugly, blurry, black, low res, unrealistic"
QK_SITES = {1: (1, 2), 2: (0, 1, 2), 3: (0, 1, 2)}       # up_blocks[i].attentions[j]: transformer blocks 8..15 of the execution order 0..15
SD_L, SD_S, SD_N_IMG = 16, 5, 2
ETA = [[0.6, 0], [1, 0.7]]


def windows(S, pnp_f_t=0.8, pnp_attn_t=0.5):
    """(conv_steps, qk_steps): the injections are live for the leading int(S f) timesteps of the backward schedule (pnp.py:50-54, 91-92)"""
    return int(S * pnp_f_t), int(S * pnp_attn_t)


def step_flags(S):
    """per backward step i: (conv live, qk live)"""
    conv, qk = windows(S)
    return [(i < conv, i < qk) for i in range(S)]


def step_rows(S, eta_zero, skip_dead_source_rows=True):
    """rows per image a backward step has to run: [u_s, u_t, c_t]; [u_t, c_t] once the source row is replayed (eta == 0) and no injection reads it"""
    return [2 if (skip_dead_source_rows and z and not (c or q)) else 3 for (c, q), z in zip(step_flags(S), eta_zero)]


class PnpUNet:
    """The oracle UNet under the three hooks.  `conv_on` / `qk_on` are this call's switches (the reference keeps a timestep list per module and
    tests `t in list`; `fired` counts what the hooked modules actually did, per call)."""

    def __init__(self, unet, n_img=1):
        self.unet, self.n, self.conv_on, self.qk_on = unet, n_img, False, False
        self.fired = {"conv": 0, "qk": 0}
        self.attn_sites = [unet.up_blocks[i].attentions[j].transformer_blocks[0].attn1 for i, js in QK_SITES.items() for j in js]
        self.conv_site = unet.up_blocks[1].resnets[1]

    # ---- hooks
    def _attn1(self, mod):
        def forward(x, encoder_hidden_states=None, attention_mask=None):
            assert encoder_hidden_states is None and attention_mask is None, "attn1 is self-attention"
            q, k, v = mod.to_q(x), mod.to_k(x), mod.to_v(x)
            if self.qk_on:                                           # target rows: Q and K of the u_s row of their image, V their own
                assert x.shape[0] == 3 * self.n
                q, k = q[:self.n].repeat(3, 1, 1), k[:self.n].repeat(3, 1, 1)
                self.fired["qk"] += 1
            q, k, v = (mod.head_to_batch_dim(a) for a in (q, k, v))
            p = (torch.einsum("bid,bjd->bij", q, k) * mod.scale).softmax(dim=-1)
            return mod.to_out[0](mod.batch_to_head_dim(torch.einsum("bij,bjd->bid", p, v)))
        return forward

    def _resnet(self, mod):
        def forward(x, temb):
            h = mod.conv1(F.silu(mod.norm1(x))) + mod.time_emb_proj(F.silu(temb))[:, :, None, None]
            h = mod.conv2(F.silu(mod.norm2(h)))
            if self.conv_on:                                         # conv2's output (bias included) of the u_s row; the shortcut stays the row's own
                assert x.shape[0] == 3 * self.n
                h = h[:self.n].repeat(3, 1, 1, 1)
                self.fired["conv"] += 1
            return (mod.conv_shortcut(x) if mod.conv_shortcut is not None else x) + h
        return forward

    @contextlib.contextmanager
    def hooked(self):
        for m in self.attn_sites:
            m.forward = self._attn1(m)
        self.conv_site.forward = self._resnet(self.conv_site)
        try:
            yield self
        finally:
            for m in self.attn_sites + [self.conv_site]:
                del m.forward                                        # back to the class's forward

    # ---- the UNet interface the oracle's loops use
    def set_ctrl(self, ctrl):
        assert ctrl is None, "plug-and-play runs without an attention controller"

    def rows3(self, sample, timestep, ctx):
        """one hooked call on rows [u_s, u_t, c_t] x n_img"""
        assert sample.shape[0] == 3 * self.n == ctx.shape[0]
        return self.unet(sample, timestep, encoder_hidden_states=ctx)["sample"]

    def __call__(self, sample, timestep, encoder_hidden_states=None):
        """rows [u_s, u_t, c_s, c_t] x n_img: the cond source rows are cut, the uncond source noise is returned in their place (pnp.py:130-146)"""
        n = self.n
        assert sample.shape[0] == 4 * n == encoder_hidden_states.shape[0]
        keep = torch.cat([torch.arange(0, 2 * n), torch.arange(3 * n, 4 * n)])
        eps = self.rows3(sample[keep], timestep, encoder_hidden_states[keep])
        return {"sample": torch.cat([eps[:2 * n], eps[:n], eps[2 * n:]])}


def pnp_sample_ref(oracle, inv, ctx_src, ctx_tgt, noise_table, edit_word_idx=None, trace=None, teacher=None):
    """`oracle` (oracle.loop.EtaInversionOracle, one image): its backward loop with the UNet under the hooks, the flags set from the step index.
    ctx_tgt = [negative prompt, target prompt].  trace entries gain "conv", "qk" (what the hooked modules did in that step) and "eps_rows"
    (the three rows the network ran).  Returns the latents [source, target]."""
    S = oracle.S
    conv_steps, qk_steps = windows(S)
    t_list = [int(t) for t in oracle.t_bwd]
    hooked = PnpUNet(oracle.unet, 1)
    plain, rows_seen = oracle.unet, []

    class Stepper:
        set_ctrl = staticmethod(hooked.set_ctrl)

        def __call__(self, sample, timestep, encoder_hidden_states=None):
            i = t_list.index(int(timestep))
            hooked.conv_on, hooked.qk_on = i < conv_steps, i < qk_steps           # (`t in timesteps[:n]`)
            before = dict(hooked.fired)
            out = hooked(sample, timestep, encoder_hidden_states=encoder_hidden_states)
            rows_seen.append({"conv": hooked.fired["conv"] > before["conv"], "qk": hooked.fired["qk"] > before["qk"],
                              "eps_rows": out["sample"][[0, 1, 3]].clone()})
            return out

    own = [] if trace is None else trace
    oracle.unet = Stepper()
    try:
        with hooked.hooked():
            z = oracle.sample(inv, ctx_src, ctx_tgt, noise_table, edit_word_idx=edit_word_idx, trace=own, teacher=teacher)
    finally:
        oracle.unet = plain
    for entry, seen in zip(own, rows_seen):
        entry.update(seen)
    return z


# ---- the SD-width case of the GPU tests (regenerated from seeds by both sides; the fixture stores probes)
def sd_case_inputs():
    """z0 (n_img,4,L,L) distinct per image, ctx_src / ctx_tgt (n_img,2,77,768): [uncond, source] and [negative, target] per image"""
    g = torch.Generator().manual_seed(47)
    z0 = 0.8 * torch.randn(SD_N_IMG, 4, SD_L, SD_L, generator=g)
    unc, neg = torch.randn(77, 768, generator=g), torch.randn(77, 768, generator=g)
    cs = torch.randn(SD_N_IMG, 77, 768, generator=g)
    ct = 0.7 * cs + 0.3 * torch.randn(SD_N_IMG, 77, 768, generator=g)         # target prompts that share most of their source prompt
    ctx_src = torch.stack([unc.expand_as(cs), cs], 1).contiguous()
    ctx_tgt = torch.stack([neg.expand_as(ct), ct], 1).contiguous()
    return z0, ctx_src, ctx_tgt


def sd_call_inputs():
    """one UNet call: latents [src, tgt, tgt] x n_img (all distinct), contexts [u_s, u_t, c_t] x n_img, timestep"""
    z0, ctx_src, ctx_tgt = sd_case_inputs()
    g = torch.Generator().manual_seed(48)
    tgt = z0 + 0.3 * torch.randn(z0.shape, generator=g)
    lat = torch.cat([z0, tgt, tgt]).contiguous()
    ctx = torch.cat([ctx_src[:, 0], ctx_tgt[:, 0], ctx_tgt[:, 1]]).contiguous()
    return lat, ctx, 601


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))
