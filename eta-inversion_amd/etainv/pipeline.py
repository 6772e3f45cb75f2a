"""Batched forward (inversion) / backward (eta-sampling) loops on the native engine.

Host logic only: timestep tables, per-step scalar coefficients and the order of C-ABI calls.  All tensors stay on
the device; nothing in the loops synchronises with the host (the best-of-n argmin runs in the eta-step kernel).

Replaces, for B independent (source, target) pairs at once (the reference handles exactly one, SURVEY E-6):
  DiffusionInversion.diffusion_forward / predict_step_forward   reference modules/inversion/diffusion_inversion.py:314-418
  EtaInversion.invert (per-step word maps + mean)               reference modules/inversion/eta_inversion.py:36-49,378-404
  EtaInversion.diffusion_backward / predict_step_backward       reference modules/inversion/eta_inversion.py:207-294
  DiffusionInversion.sample batch layout                        reference modules/inversion/diffusion_inversion.py:462-528
  EdictInversion.predict_step_forward / predict_step_backward   reference modules/inversion/edict_inversion.py:393-420 (EdictLoop)
  DDPMInversion.diffusion_forward / diffusion_backward          reference modules/inversion/ddpm_inversion.py:71-104,168-177 (DdpmLoop)
"""
import functools
import os

import numpy as np
import torch

from . import _capi
from .engine import AttnControl
from .flops import ddpm_unet_rows, edict_unet_rows, exit_share
from .plan import FULL, LAYOUTS, ddpm_guided, plan_backward, plan_ddpm_chunks

NUM_TRAIN = 1000


def alphas_cumprod() -> np.ndarray:
    """scaled_linear 0.00085..0.012, fp32 cumprod (reference modules/models/__init__.py:134)."""
    betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, NUM_TRAIN, dtype=torch.float32) ** 2
    return torch.cumprod(1.0 - betas, dim=0).numpy().astype(np.float64)


def eta_table(eta=(0.0, 0.4)) -> np.ndarray:
    """etas[1000] by raw timestep (reference modules/inversion/eta_inversion.py:52-58,121-139), without eval()."""
    if not isinstance(eta, (tuple, list)):
        eta = (eta, eta)
    ts = np.linspace(0, 1, NUM_TRAIN)
    if len(eta) == 3 or isinstance(eta[0], (tuple, list)):
        (x1, y1), (x2, y2) = eta[0], eta[1]
        p = eta[2] if len(eta) == 3 else 1
        a = (y2 - y1) / (x2 - x1) ** p
        etas = a * (np.clip(ts, x1, x2) - x1) ** p + y1
    else:
        etas = np.linspace(eta[0], eta[1], NUM_TRAIN)
    return np.clip(etas, 0, None)


def _env_on(name):
    """A/B switches: set and not "" / "0" """
    return os.environ.get(name, "0") not in ("", "0")


def attn_layer_selection(L, attn_res=None, attn_from_where=("up", "down")):
    """(res_div, layer mask) of etainv_maps_configure / etainv_maps_word_maps_ex for the reference's (attn_res, attn_from_where)"""
    attn_res = L // 4 if attn_res is None else int(attn_res)
    if attn_res <= 0 or L % attn_res or L // attn_res not in (2, 4, 8):
        raise NotImplementedError(f"attn_res must be L/2, L/4 or L/8 (cross layers exist at those sizes only), got {attn_res} at L = {L}")
    div = L // attn_res
    if div == 8:                                                # ptp.py:293-294 (`res == 8` at the reference's 64 x 64 latents)
        return div, 0x01
    where = set(attn_from_where)
    if not where <= {"up", "down", "mid"}:
        raise ValueError(f"attn_from_where entries must be 'up', 'down' or 'mid', got {sorted(where)}")
    mask = (0x03 if "down" in where else 0) | (0x1c if "up" in where else 0)
    if mask == 0:
        raise ValueError(f"attn_from_where {sorted(where)} has no cross layer with {attn_res}^2 tokens (the reference fails in torch.cat, ptp.py:301)")
    return div, mask


class _MaskSource:
    """The eta mask of one `EtaLoop.sample` call (reference eta_inversion.py:164-201): `static` maps, the raw map of a source at a step, get_mask's tail"""

    def __init__(self, loop, inv, edit_word, edit_word_tgt, gt_mask, ptp):
        self.loop, self.inv = loop, inv
        L, B, dev = loop.L, inv["latents"].shape[1], inv["latents"].device
        self.idx = edit_word.to(dev).long().reshape(B, 1, 1, 1).expand(B, 1, L, L)
        self.mode = 2 if loop.mask_thres is None or loop.mask_pow is not None or loop.mask_eta != "fwd_mean" else 1   # 2: the map is the per-pixel eta multiplier
        sources = {loop.mask_eta, loop.mask_dirinv} - {None}
        if any(sname.startswith("bwd") for sname in sources):                        # maps of the backward-pass store (eta_inversion.py:176-183)
            assert ptp is not None, "bwd_* masks read the prompt-to-prompt controller's maps"
            token = lambda word: (word.to(dev).int() + 1).reshape(B, 1).contiguous()
            self.tok_s, self.tok_t = token(edit_word), token(edit_word_tgt if edit_word_tgt is not None else edit_word)
            self.map_s, self.map_t = (torch.empty(B, 1, L, L, dtype=torch.float32, device=dev) for _ in range(2))
        self.static = {}
        if "gt" in sources:
            assert gt_mask is not None, "a 'gt' mask source needs the ground-truth mask (B,L,L)"
            self.static["gt"] = gt_mask.to(dev).float().reshape(B, L, L)
        if "fwd_mean" in sources:
            self.static["fwd_mean"] = inv["maps_mean"].gather(1, self.idx).reshape(B, L, L)

    def shaped(self, m):                                                            # get_mask tail, eta_inversion.py:196-201: threshold, then power
        m = m if self.loop.mask_thres is None else (m > self.loop.mask_thres).to(m.dtype)
        return (m if self.loop.mask_pow is None else torch.pow(m, self.loop.mask_pow)).contiguous()

    def src_map(self, name, i):                                                     # raw map of one source at backward step i (eta_inversion.py:164-183)
        loop, (B, _, L, _) = self.loop, self.idx.shape
        if name in self.static:
            return self.static[name]
        if name == "fwd":                                                           # map of THIS timestep (t_bwd[i] == t_fwd[S-1-i])
            return self.inv["maps_steps"][loop.S - 1 - i].gather(1, self.idx).reshape(B, L, L)
        if name != "bwd_target":                                                    # average over the i+1 backward steps done, this one included
            loop.e.word_maps_ex(B, self.tok_s, i + 1, 0, loop.attn_layer_mask, self.map_s)
        if name != "bwd_source":
            loop.e.word_maps_ex(B, self.tok_t, i + 1, 1, loop.attn_layer_mask, self.map_t)
        m = self.map_s if name == "bwd_source" else self.map_t if name == "bwd_target" else torch.maximum(self.map_s, self.map_t)
        return m.reshape(B, L, L)


class EtaLoop:

    def __init__(self, engine, S=50, guidance_scale_bwd=7.5, guidance_scale_fwd=1.0, eta=(0.0, 0.4), noise_sample_count=10,
                 use_mask=True, mask_thres=0.2, skip_uncond_fwd=True, steps_offset=0, mask_eta="fwd_mean", mask_pow=None, target_dirinv=None,
                 mask_dirinv=None, skip_dead_source_rows=True, attn_res=None, attn_from_where=("up", "down"), regularizer=None):
        self.e, self.S, self.L = engine, S, engine.L
        # NoiseRegularizer or None: `invert` then pushes every guided noise towards white noise before the DDIM step (regularised DDIM inversion,
        # reference modules/inversion/regularized_diffusion_inversion.py:116-137), CFG combine, regularisation and step in one launch
        self.regularizer = regularizer
        # which cross layers the eta mask's word maps average (mask_mode_cfg attn_res / attn_from_where, eta_inversion.py:161-162; aggregate_attention
        # ptp.py:288-303: the layers with res^2 tokens of the named locations, `res == 8` -> the mid block whatever from_where says)
        self.attn_div, self.attn_layer_mask = attn_layer_selection(self.L, attn_res, attn_from_where)
        if use_mask and self.attn_div != 4 and any(str(m).startswith("bwd") for m in (mask_eta, mask_dirinv)):
            raise NotImplementedError("bwd_* mask sources with attn_res != L/4: the backward pass keeps the (L/4)^2 store LocalBlend reads")
        # guidance_scale_fwd may be a (start, end) pair: linspace over the 1000 training timesteps, indexed by t (eta_inversion.py:108-110,325-326)
        self.g_fwd_table = np.linspace(guidance_scale_fwd[0], guidance_scale_fwd[1], NUM_TRAIN) if isinstance(guidance_scale_fwd, (tuple, list)) else None
        self.g_bwd, self.g_fwd = float(guidance_scale_bwd), (1.0 if self.g_fwd_table is not None else float(guidance_scale_fwd))
        self.ac = alphas_cumprod()
        self.delta = NUM_TRAIN // S
        self.t_bwd = ((np.arange(S) * self.delta)[::-1] + steps_offset).astype(np.int64)
        self.t_fwd = self.t_bwd[::-1].copy()
        self.etas = eta_table(eta)
        self.n_cand = noise_sample_count
        self.use_mask, self.mask_thres = use_mask, mask_thres
        # non-default eta-mask modes (reference eta_inversion.py:164-201): source of the map (fwd_mean | fwd | gt), thres None = soft, pow
        self.mask_eta, self.mask_pow = mask_eta, mask_pow
        # target_dirinv w: x_tgt += w (1 - mask_dirinv) (x_prev_src - x_src_new)  (eta_inversion.py:251-256); mask_dirinv names its own map
        # source (any of the mask_eta sources) or None
        self.target_dirinv, self.mask_dirinv = target_dirinv, mask_dirinv
        assert target_dirinv is None or use_mask, "target_dirinv is part of the masked update"
        # u + 1*(c - u) == c up to rounding: the uncond half of the forward pass is dead work when g_fwd == 1
        self.skip_uncond_fwd = skip_uncond_fwd and self.g_fwd == 1.0 and self.g_fwd_table is None
        if regularizer is not None and regularizer.L != self.L:
            raise ValueError(f"the regulariser was built for {regularizer.L} x {regularizer.L} latents, the engine runs {self.L} x {self.L}")
        # Backward steps with eta(t) == 0 (30 of 50 with the paper's eta [[0.6, 0], [1, 0.7]]) REPLAY the source row from the inversion trajectory (eta_inversion.py:
        # 247-249); its guided noise only picks a noise sample that is then multiplied by eta sigma = 0 (:232, :330-375), so eps(uncond source) is dead work and those
        # steps run fewer rows (which ones: etainv.plan).  Like skip_uncond_fwd an identity of the reference's arithmetic, the source row one rounding apart at most
        # (SURVEY E-11), not an approximation; skip_dead_source_rows=False runs the reference's row count.  The environment variables are A/B switches.
        self.skip_dead_source_rows = skip_dead_source_rows and target_dirinv is None and not _env_on("ETAINV_NO_DEAD_ROW_SKIP")
        # ... and the cond source row of such a step leaves the network early once nothing is injected from it (etainv_attn_ctrl.src_exit_block)
        self.src_exit = self.skip_dead_source_rows and not _env_on("ETAINV_NO_SRC_EXIT")
        self.src_exit_9_only = _env_on("ETAINV_SRC_EXIT_9_ONLY")   # A/B: no exit while the self-replace runs
        # share of a sample-forward's FLOPs a row has run when it leaves after transformer block 9 / 12, at THIS latent size (0.509 / 0.716 at L = 64)
        self.SRC_EXIT_SHARE, self.SRC_EXIT_SHARE_12 = exit_share(self.L, 9), exit_share(self.L, 12)
        self.rows_executed = 0                                   # UNet sample-forwards issued by invert / sample since construction (bench accounting)
        self.lib = engine.lib

    def _alpha(self, tau):
        tau = min(int(tau), NUM_TRAIN - 1)
        return float(self.ac[tau]) if tau >= 0 else float(self.ac[0])

    # ---------------------------------------------------------------- forward / inversion
    def invert(self, z0, ctx_src, tokens=None, teacher=None):
        """z0 (B,4,L,L) fp32; ctx_src (B,2,77,768) = [uncond, cond] per image; tokens (B,W) int32 token index of each
        whitespace word (first occurrence + 1).  Returns latents (S+1,B,4,L,L) and the mean word maps (B,W,L,L); with a regulariser also
        "noise_preds" (S,B,4,L,L), the regularised noise of every step.
        teacher (S+1,B,4,L,L), tests only: step j reads teacher[j] instead of its own previous output (teacher-forced parity:
        every step is compared with the oracle on the oracle's input, so rounding is not amplified by the recursion)."""
        e, S, L = self.e, self.S, self.L
        B = z0.shape[0]
        dev = z0.device
        lat = torch.empty(S + 1, B, 4, L, L, dtype=torch.float32, device=dev)
        lat[0].copy_(z0)
        if self.skip_uncond_fwd:
            ctx = ctx_src[:, 1].contiguous().float()
        else:
            ctx = torch.cat([ctx_src[:, 0], ctx_src[:, 1]]).contiguous().float()
        rows = ctx.shape[0]
        eps_all = torch.empty(rows, 4, L, L, dtype=torch.float32, device=dev)
        eps = eps_all if self.skip_uncond_fwd else torch.empty(B, 4, L, L, dtype=torch.float32, device=dev)
        reg = self.regularizer
        eps_reg = torch.empty(S, B, 4, L, L, dtype=torch.float32, device=dev) if reg is not None else None
        maps_mean = maps_steps = None
        ctrl = None
        if self.use_mask:
            assert tokens is not None
            maps_mean = torch.zeros(B, tokens.shape[1], L, L, dtype=torch.float32, device=dev)
            if "fwd" in (self.mask_eta, self.mask_dirinv):                        # per-step maps, keyed by step (eta_inversion.py:44-49,168)
                maps_steps = torch.zeros(S, B, tokens.shape[1], L, L, dtype=torch.float32, device=dev)
            ctrl = AttnControl(mode=_capi.ATTN_STORE, n_img=B, store_maps=True)
            if e.map_div != self.attn_div:
                e.maps_configure(self.attn_div)                                   # (clears the store)
            else:
                e.maps_reset()
        n = B * 4 * L * L
        st = _capi.stream_ptr()
        with e.cached_context():                               # one unchanged context tensor for all S calls
            for j, t in enumerate(self.t_fwd):
                x_in = lat[j] if teacher is None else teacher[j].contiguous()
                e.unet(x_in, int(t), ctx, ctrl, out=eps_all)
                self.rows_executed += rows
                a_from, a_to = self._alpha(int(t) - self.delta), self._alpha(int(t))   # "sameshift" (scheduling_ddim_inverse.py:127-131)
                g = float(self.g_fwd_table[int(t)]) if self.g_fwd_table is not None else self.g_fwd
                if reg is not None:
                    if self.skip_uncond_fwd:                   # one row per image: the noise already is the guided one
                        reg.run(self.lib, None, eps_all, 1.0, eps_reg[j], x_in, a_from, a_to, lat[j + 1], B, st)
                    else:
                        reg.run(self.lib, eps_all[:B], eps_all[B:], g, eps_reg[j], x_in, a_from, a_to, lat[j + 1], B, st)
                else:
                    if not self.skip_uncond_fwd:
                        _capi.check(self.lib.etainv_cfg_combine(_capi.ptr(eps_all[:B]), _capi.ptr(eps_all[B:]), g, _capi.ptr(eps), n,
                                                                _capi.F32, st))
                    _capi.check(self.lib.etainv_ddim_step(_capi.ptr(x_in), _capi.ptr(eps), a_from, a_to, _capi.ptr(lat[j + 1]), n, _capi.F32, st))
                if self.use_mask:
                    e.word_maps_ex(B, tokens, j + 1, 0, self.attn_layer_mask, maps_mean, accumulate=True, scale=1.0 / S)
                    if maps_steps is not None:
                        e.word_maps_ex(B, tokens, j + 1, 0, self.attn_layer_mask, maps_steps[j], accumulate=False, scale=1.0)
        res = {"latents": lat, "maps_mean": maps_mean, "maps_steps": maps_steps}
        if reg is not None:
            res["noise_preds"] = eps_reg
        return res

    # ---------------------------------------------------------------- backward / eta sampling
    def sample(self, inv, ctx_src, ctx_tgt, noise, edit_word=None, ptp=None, masactrl=None, trace=None, gt_mask=None, edit_word_tgt=None,
               teacher=None, pnp=None):
        """noise (S,n_cand,4,L,L) fp32: the candidates of every step (reference draws them from a generator reseeded
        per image, eta_inversion.py:156,276, so all images share the table).  edit_word (B,) index into the word maps.
        ptp: PtpTables or None; masactrl: (start_step, first_block) or None; pnp: (conv_steps, qk_steps) or None -- plug-and-play, the number of
        leading backward steps with the feature / the Q,K injection (reference modules/utils/pnp.py:50-54: int(S * 0.8), int(S * 0.5)); ctx_tgt[:, 0] then
        is the negative-prompt row.  At most one of ptp / masactrl / pnp.  Returns latents (2B,4,L,L) [src.., tgt..].
        teacher (S,2B,4,L,L), tests only: step i starts from teacher[i] (see invert)."""
        e, S, L, lat_inv = self.e, self.S, self.L, inv["latents"]
        B, dev = lat_inv.shape[1], lat_inv.device
        if sum(c is not None for c in (ptp, masactrl, pnp)) > 1:
            raise ValueError("ptp, masactrl and pnp are exclusive: one attention coupling per backward pass")
        steps = plan_backward(S, self.t_bwd, self.etas, self.ac, self.delta, L, B, self.skip_dead_source_rows, self.src_exit, self.src_exit_9_only, ptp, masactrl, pnp)
        roles = {"u_s": ctx_src[:, 0], "u_t": ctx_tgt[:, 0], "c_s": ctx_src[:, 1], "c_t": ctx_tgt[:, 1]}

        @functools.lru_cache(maxsize=None)
        def buffers(name):                                      # (context rows, noise rows, their eu and ec groups) of a layout, built when it first runs
            lay = LAYOUTS[name]
            eps = torch.empty(len(lay.roles) * B, 4, L, L, dtype=torch.float32, device=dev)
            return torch.cat([roles[r] for r in lay.roles]).contiguous().float(), eps, eps[lay.eu * B:(lay.eu + 1) * B], eps[lay.ec * B:(lay.ec + 1) * B]
        eps_all = buffers(FULL)[1]                                                 # the eta step reads the reference's four row groups, whatever ran
        x = torch.cat([lat_inv[S], lat_inv[S]]).contiguous()
        x_new = torch.empty_like(x)
        best, scratch = torch.zeros(B, dtype=torch.int32, device=dev), torch.empty(B * 16 * 64, dtype=torch.float32, device=dev)
        masks = _MaskSource(self, inv, edit_word, edit_word_tgt, gt_mask, ptp) if self.use_mask else None
        mask_map, mask_mode = None, (masks.mode if masks is not None else 0)
        if ptp is not None:
            if e.map_div != 4:
                e.maps_configure(4)                                                  # LocalBlend and the bwd_* sources read the (L/4)^2 layers
            else:
                e.maps_reset()
        losses = torch.zeros(B, self.n_cand, dtype=torch.float32, device=dev) if trace is not None else None   # per-candidate losses of the best-of-n step (traces only)
        eps_t = torch.empty(B, 4, L, L, dtype=torch.float32, device=dev)
        st = _capi.stream_ptr()
        with e.cached_context():                               # the context tensor of a layout stays unchanged over all its calls
            for i, s in enumerate(steps):
                lay = LAYOUTS[s.layout]
                ctrl = None
                if lay.ctrl and ptp is not None:
                    ctrl = AttnControl(mode=_capi.ATTN_PTP, n_img=B, store_maps=True, mapper=ptp.mapper if s.edit else None, alphas=ptp.alphas,
                                       replace_mat=ptp.replace_mat if s.edit else None, equalizer=ptp.equalizer, cross_alpha=ptp.cross_alpha[i],
                                       self_replace_active=s.self_replace_active, self_max_tokens=(L // 2) ** 2)
                    ctrl.c.first_row, ctrl.c.src_exit_block = s.first_row, s.src_exit_block
                elif lay.ctrl and masactrl is not None:
                    ctrl = AttnControl(mode=_capi.ATTN_MASA, n_img=B, masa_active=s.masa_active, masa_first_block=masactrl[1])
                elif lay.ctrl and pnp is not None:
                    ctrl = AttnControl(mode=_capi.ATTN_PNP, n_img=B, pnp_qk_active=s.pnp_qk_active, pnp_conv_active=s.pnp_conv_active)
                if teacher is not None:
                    x.copy_(teacher[i])
                ctx, eps, eu, ec = buffers(s.layout)
                lat = x if lay.latents == ("src", "tgt") else x[B:] if lay.latents == ("tgt",) else torch.cat([x[:B] if side == "src" else x[B:] for side in lay.latents])
                e.unet(lat, s.t, ctx, ctrl, out=eps)
                self.rows_executed += B * s.cost
                if s.replay:                                                            # eta == 0: plain DDIM step of the target, the source row is replayed
                    _capi.check(self.lib.etainv_cfg_combine(_capi.ptr(eu), _capi.ptr(ec), self.g_bwd, _capi.ptr(eps_t), B * 4 * L * L, _capi.F32, st))
                    _capi.check(self.lib.etainv_ddim_eta_step(_capi.ptr(x[B:]), _capi.ptr(eps_t), 0.0, None, 0, None, s.a_t, s.a_p, s.var, B, 4, L * L, _capi.ptr(x_new[B:]), _capi.F32, st))
                    x_new[:B].copy_(lat_inv[S - 1 - i])
                    best.zero_()                                                        # (the reference's argmin over NaN losses: index 0)
                else:
                    if pnp is not None:                                                 # u_s stands in for the cut c_s: rows [0, 1, 0, 2] (pnp.py:146)
                        eps_all.view(4, B, 4, L, L).copy_(eps.view(3, B, 4, L, L)[[0, 1, 0, 2]])
                    dmap = None
                    if masks is not None:
                        raw = masks.src_map(self.mask_eta, i)
                        mask_map = masks.shaped(raw) if mask_mode == 2 else raw.contiguous()   # mode 1: the kernel thresholds the raw forward-mean map
                        if self.target_dirinv is not None and self.mask_dirinv is not None:   # 1 - shaped map of the mask_dirinv source (eta_inversion.py:234-256)
                            dmap = (1.0 - masks.shaped(raw if self.mask_dirinv == self.mask_eta else masks.src_map(self.mask_dirinv, i))).contiguous()
                    _capi.check(self.lib.etainv_eta_backward_step_ex(
                        _capi.ptr(x), _capi.ptr(eps_all), self.g_bwd, _capi.ptr(lat_inv[S - 1 - i]), _capi.ptr(noise[i]), self.n_cand,
                        s.eta, _capi.ptr(mask_map), float(self.mask_thres or 0.0), mask_mode, s.a_t, s.a_p, s.var, B, 4, L * L,
                        _capi.ptr(x_new), None, _capi.ptr(best), _capi.ptr(losses), _capi.ptr(scratch), _capi.F32, float(self.target_dirinv or 0.0), _capi.ptr(dmap), st))
                x, x_new = x_new, x
                if s.blend:
                    e.local_blend(x, B, ptp.blend_alpha, 0.3)                       # LocalBlend, reference ptp.py:31-47
                if trace is not None:
                    # "eps_rows": the rows with an output this step ran, B per name of "layout"; "eps_all" (4 B rows) and "losses": eta steps only
                    trace.append({"t": s.t, "latent": x.clone(), "best": best.clone(), "eps_all": None if s.replay else eps_all.clone(),
                                  "eps_rows": eps[:lay.n_out * B].clone(), "layout": s.trace_layout, **({} if s.replay else {"losses": losses.clone()})})
        return x


class PtpTables:
    """Device tables of one prompt-to-prompt edit per image (what ptp.make_controller builds on the host,
    reference modules/utils/ptp.py:306-320)."""

    def __init__(self, mapper, alphas, cross_alpha, self_replace_steps, S, equalizer=None, blend_alpha=None, replace_mat=None,
                 device="cuda"):
        T = lambda a, dt: None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(device).contiguous()
        self.mapper = T(mapper, torch.int32)              # (B,77)
        self.alphas = T(alphas, torch.float32)            # (B,77)
        self.equalizer = T(equalizer, torch.float32)      # (B,77)
        self.replace_mat = T(replace_mat, torch.float32)  # (B,77,77)
        self.blend_alpha = T(blend_alpha, torch.float32)  # (B,2,77)
        self.cross_alpha = T(cross_alpha, torch.float32)  # (S+1,B,77)
        # steps whose cross_replace_alpha row is all zero: the cross edit is the identity there (rep * 0 + 1 * own, reference ptp.py:228) -- the loop
        # then runs the plain cross-attention launch for the cond-target rows too (no source-probability recomputation); the map store stays on
        ca = np.asarray(cross_alpha, dtype=np.float32)
        self.cross_active = (ca.reshape(ca.shape[0], -1) != 0).any(1)
        if isinstance(self_replace_steps, float):
            self_replace_steps = (0, self_replace_steps)
        self.self_lo, self.self_hi = int(S * self_replace_steps[0]), int(S * self_replace_steps[1])


def noise_table(S, n, L, seed=0, device="cuda"):
    """CPU torch generator, reseeded per image like the reference (eta_inversion.py:276): one table for all images."""
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randn((n, 1, 4, L, L), generator=g) for _ in range(S)]).reshape(S, n, 4, L, L).to(device)


# ---------------------------------------------------------------- regularised DDIM inversion (reference modules/inversion/regularized_diffusion_inversion.py)
def regdiff_level_sizes(L):
    """sides of auto_corr_loss's average-pool pyramid (:61-68): the loss at a level, then pool while the level is above 8"""
    sizes = [int(L)]
    while sizes[-1] > 8:
        sizes.append(sizes[-1] // 2)
    return sizes


def regdiff_shift_table(L, num_reg_steps=5, num_ac_rolls=5, lambda_ac=20.0, generator=None, seed=0):
    """int32 [num_reg_steps * num_ac_rolls][4][levels]: the roll amounts of regularize_noise_pred (:86-114) in the order the reference draws
    them -- autocorrelation step, channel, level from fine to coarse, each one `torch.randint(0, s // 2, ())` (:62).  generator None: a fresh
    CPU generator with `seed`; the reference reseeds to 0 at every inversion step (:117), so one table serves all steps.  Nothing is drawn
    with lambda_ac <= 0 (:99)."""
    sizes = regdiff_level_sizes(L)
    n = int(num_reg_steps) * int(num_ac_rolls) if lambda_ac > 0 else 0
    g = generator if generator is not None else torch.Generator().manual_seed(seed)
    table = np.zeros((n, 4, len(sizes)), dtype=np.int32)
    for a in range(n):
        for c in range(4):
            for k, s in enumerate(sizes):
                table[a, c, k] = torch.randint(0, s // 2, (), generator=g).item()
    return table


class NoiseRegularizer:
    """The four parameters of the noise regularisation and the device shift table (built once), and the call of etainv_noise_regularize."""

    def __init__(self, L, lambda_ac=20.0, lambda_kl=20.0, num_reg_steps=5, num_ac_rolls=5, device="cuda", seed=0):
        self.L, self.lambda_ac, self.lambda_kl = int(L), float(lambda_ac), float(lambda_kl)
        self.num_reg_steps, self.num_ac_rolls = int(num_reg_steps), int(num_ac_rolls)
        self.device, self.seed = device, seed
        self._shifts, self._built = None, False

    def table(self, generator=None):
        """device table of the draws of `generator`, or (built once) of a fresh generator with the regulariser's seed; None when nothing is drawn"""
        if generator is None and self._built:
            return self._shifts
        host = regdiff_shift_table(self.L, self.num_reg_steps, self.num_ac_rolls, self.lambda_ac, generator, self.seed)
        dev = torch.from_numpy(host).to(self.device).contiguous() if host.size else None
        if generator is None:
            self._shifts, self._built = dev, True
        return dev

    def run(self, lib, eps_u, eps_c, g, eps_out, x, a_from, a_to, x_out, n_img, stream, shifts=None):
        """eps_u / x None: no CFG combine / no DDIM step (see include/etainv.h)"""
        shifts = shifts if shifts is not None else self.table()
        _capi.check(lib.etainv_noise_regularize(_capi.ptr(eps_u), _capi.ptr(eps_c), float(g), _capi.ptr(eps_out), _capi.ptr(x), float(a_from), float(a_to),
                                                _capi.ptr(x_out), int(n_img), self.L, _capi.ptr(shifts), self.num_reg_steps, self.num_ac_rolls,
                                                self.lambda_ac, self.lambda_kl, stream))


# ---------------------------------------------------------------- proximal guidance (reference modules/inversion/proximal_negative_prompt_inversion.py)
class ProximalGuidance:
    """The parameters of proximal_guidance (:61-128), the rank split of its torch.quantile, and the call of etainv_prox_guidance.
    prox None: plain CFG; "l0" / "l1": the two shrinkages; anything else is refused at the call, as the reference does.  quantile > 0: the
    threshold is that quantile of |eps_c - eps_u| over a group; quantile <= 0: the fixed threshold -quantile."""
    MODES = {None: 0, "l0": 1, "l1": 2}

    def __init__(self, L, prox="l0", quantile=0.7):
        if quantile > 1:
            raise ValueError(f"quantile must be at most 1 (a quantile of |eps_c - eps_u|) or <= 0 (a fixed threshold), got {quantile}")
        self.L, self.prox, self.quantile = int(L), prox, float(quantile)

    @staticmethod
    def rank_split(n, q):
        """(k, w) of torch.quantile(x, q) over n fp32 values, linear interpolation: rank = float32(q) * (n - 1) in fp32, k = floor(rank),
        w = rank - k; the quantile is lerp(sorted[k], sorted[min(k + 1, n - 1)], w)"""
        rank = np.float32(q) * np.float32(n - 1)
        k = min(int(np.floor(rank)), n - 1)
        return k, float(np.float32(rank - np.float32(k)))

    def run(self, lib, eps_u, eps_c, g, eps_out, x, a_from, a_to, x_out, n_groups, rows_per_group, stream=None, thr_out=None):
        """x None: no DDIM step; stream None: torch's current stream (see include/etainv.h)"""
        if self.prox not in self.MODES:
            raise NotImplementedError(f"proximal guidance '{self.prox}' is not defined (None, 'l0', 'l1')")
        mode = self.MODES[self.prox]
        use_rank, k, w, thr = 0, 0, 0.0, 0.0
        if mode and self.quantile > 0:
            use_rank = 1
            k, w = self.rank_split(int(rows_per_group) * 4 * self.L * self.L, self.quantile)
        elif mode:
            thr = 0.0 - self.quantile
        _capi.check(lib.etainv_prox_guidance(_capi.ptr(eps_u), _capi.ptr(eps_c), float(g), mode, use_rank, k, w, thr, _capi.ptr(eps_out), _capi.ptr(x),
                                             float(a_from), float(a_to), _capi.ptr(x_out), _capi.ptr(thr_out), int(n_groups), int(rows_per_group),
                                             self.L, stream if stream is not None else _capi.stream_ptr()))


# ---------------------------------------------------------------- EDICT host tables (reference modules/inversion/edict_inversion.py)
def edict_timesteps(S, init_image_strength=1.0):
    """(forward, backward) timesteps that run: the scheduler's leading-spaced S timesteps with the t_limit = S - int(S strength) noisiest
    ones cut off both ways (:258,422-428)"""
    t_bwd = (np.arange(S) * (NUM_TRAIN // S))[::-1].astype(np.int64)
    t_limit = S - int(S * init_image_strength)
    return t_bwd[::-1][:S - t_limit].copy(), t_bwd[t_limit:].copy()


def edict_alpha(ac, final, t):
    """get_alpha_and_beta (:82-111) on the fp32 table `ac` (torch): a long timestep indexes it; the float `t - 1000 / S` takes
    final_alpha_cumprod below 0 and otherwise `low * rem + high * (1 - rem)` -- the reference's weights, reversed as they are"""
    if t.dtype == torch.long:
        return ac[t]
    if t < 0:
        return final
    low, high = t.floor().long(), t.ceil().long()
    rem = t - low
    return ac[low] * rem + ac[high] * (1 - rem)


def edict_coefficients(ac, final, t, S, inverse):
    """(a, b) of x' = a x + b eps at timestep t, in fp32 tensor arithmetic like the reference's scheduler steps (:157-173 denoising, :207-222
    inversion): q = sqrt(abar_t / abar_prev), prev = t - 1000 / S as a float"""
    t = torch.as_tensor(int(t), dtype=torch.long)
    prev = t - NUM_TRAIN / S
    a_t, a_p = edict_alpha(ac, final, t), edict_alpha(ac, final, prev)
    q = (a_t / a_p) ** 0.5
    if inverse:
        a, b = q, (1 - a_t) ** 0.5 - q * (1 - a_p) ** 0.5
    else:
        a = 1.0 / q
        b = (1 - a_p) ** 0.5 - a * (1 - a_t) ** 0.5
    return float(a), float(b)


def edict_order(i, S, is_fwd, leapfrog_steps=True):
    """iter_latent_pair (:288-315): the pair member updated first and second at step index i of the (truncated) timestep list; S is the full
    number of scheduler timesteps"""
    off = ((S - i) % 2 if leapfrog_steps else 1) if is_fwd else i % 2
    return off, 1 - off


class EdictLoop:
    """EDICT (coupled latent pair) for B images at once: per step two UNet calls, the second on the first's output, and the fused
    etainv_edict_* kernels between them.  All tables (timesteps, coefficients, update order) are host scalars computed once."""

    def __init__(self, engine, S=50, guidance_scale_fwd=3.0, guidance_scale_bwd=3.0, mix_weight=0.93, leapfrog_steps=True, init_image_strength=1.0):
        if not 0.0 < float(mix_weight) <= 1.0:
            raise ValueError(f"mix_weight must be in (0, 1], got {mix_weight}")
        self.e, self.S, self.L = engine, S, engine.L
        self.g_fwd, self.g_bwd, self.p = float(guidance_scale_fwd), float(guidance_scale_bwd), float(mix_weight)
        self.leapfrog_steps, self.init_image_strength = leapfrog_steps, init_image_strength
        self.t_fwd, self.t_bwd = edict_timesteps(S, init_image_strength)
        ac = torch.as_tensor(alphas_cumprod().astype(np.float32))
        self.coef_fwd = [edict_coefficients(ac, ac[0], t, S, True) for t in self.t_fwd]
        self.coef_bwd = [edict_coefficients(ac, ac[0], t, S, False) for t in self.t_bwd]
        self.order_fwd = [edict_order(i, S, True, leapfrog_steps) for i in range(len(self.t_fwd))]
        self.order_bwd = [edict_order(i, S, False) for i in range(len(self.t_bwd))]
        self.rows_executed = 0
        self.lib = engine.lib

    @staticmethod
    def _rows(ctx_u, ctx_c, g):
        """context rows of predict_noise (diffusion_inversion.py:263-286): scale 0 / 1 run one half, no guidance arithmetic"""
        if g in (0.0, 1.0):
            return (ctx_c if g == 1.0 else ctx_u).contiguous().float(), False
        return torch.cat([ctx_u, ctx_c]).contiguous().float(), True

    def invert(self, z0, ctx_src, guidance_scale_fwd=None):
        """z0 (B,4,L,L) fp32; ctx_src (B,2,77,768) = [uncond, cond] per image.  Returns the pair trajectory (S'+1,2,B,4,L,L): [0] = two copies of z0."""
        e, L = self.e, self.L
        g = float(guidance_scale_fwd or self.g_fwd)
        B, dev = z0.shape[0], z0.device
        n_steps = len(self.t_fwd)
        lat = torch.empty(n_steps + 1, 2, B, 4, L, L, dtype=torch.float32, device=dev)
        lat[0, 0].copy_(z0)
        lat[0, 1].copy_(z0)
        ctx, guided = self._rows(ctx_src[:, 0], ctx_src[:, 1], g)
        rows = ctx.shape[0]
        eps_all = torch.empty(rows, 4, L, L, dtype=torch.float32, device=dev)
        eps_u, eps_c = (_capi.ptr(eps_all[:B]), _capi.ptr(eps_all[B:])) if guided else (None, _capi.ptr(eps_all))
        n = B * 4 * L * L
        st = _capi.stream_ptr()
        with e.cached_context():
            for j, t in enumerate(self.t_fwd):
                pair = lat[j + 1]
                pair.copy_(lat[j])
                _capi.check(self.lib.etainv_edict_mix(_capi.ptr(pair[0]), _capi.ptr(pair[1]), self.p, 1, n, _capi.F32, st))
                a, b = self.coef_fwd[j]
                for k in self.order_fwd[j]:
                    e.unet(pair[1 - k], int(t), ctx, None, out=eps_all)
                    self.rows_executed += rows
                    _capi.check(self.lib.etainv_edict_couple(_capi.ptr(pair[k]), eps_u, eps_c, g, a, b, _capi.ptr(pair[k]), n, _capi.F32, st))
        return {"latents": lat}

    def sample(self, inv, ctx_list):
        """inv: result of `invert`; ctx_list: one (B,2,77,768) context per prompt -- [src, tgt] gives UNet rows [u_src x B, u_tgt x B, c_src x B,
        c_tgt x B] over the latents [src x B, tgt x B], one prompt gives [u x B, c x B].  Returns the final pair (2, n B, 4, L, L)."""
        e, L = self.e, self.L
        last = inv["latents"][-1]
        n_p, B, dev = len(ctx_list), last.shape[1], last.device
        pair = torch.stack([torch.cat([last[m]] * n_p) for m in range(2)]).contiguous()
        ctx, guided = self._rows(torch.cat([c[:, 0] for c in ctx_list]), torch.cat([c[:, 1] for c in ctx_list]), self.g_bwd)
        rows, nb = ctx.shape[0], n_p * B
        eps_all = torch.empty(rows, 4, L, L, dtype=torch.float32, device=dev)
        eps_u, eps_c = (_capi.ptr(eps_all[:nb]), _capi.ptr(eps_all[nb:])) if guided else (None, _capi.ptr(eps_all))
        n = nb * 4 * L * L
        st = _capi.stream_ptr()
        x, y = _capi.ptr(pair[0]), _capi.ptr(pair[1])
        with e.cached_context():
            for i, t in enumerate(self.t_bwd):
                a, b = self.coef_bwd[i]
                k1, k2 = self.order_bwd[i]
                e.unet(pair[1 - k1], int(t), ctx, None, out=eps_all)
                _capi.check(self.lib.etainv_edict_couple(_capi.ptr(pair[k1]), eps_u, eps_c, self.g_bwd, a, b, _capi.ptr(pair[k1]), n, _capi.F32, st))
                e.unet(pair[1 - k2], int(t), ctx, None, out=eps_all)
                _capi.check(self.lib.etainv_edict_couple_mix(x, y, k2, eps_u, eps_c, self.g_bwd, a, b, self.p, n, _capi.F32, st))
                self.rows_executed += 2 * rows
        return pair

    def expected_rows(self, B, n_prompts, guidance_scale_fwd=None):
        """UNet sample-forwards of one invert + one sample (flops.edict_unet_rows)"""
        return edict_unet_rows(len(self.t_fwd), len(self.t_bwd), B, n_prompts, float(guidance_scale_fwd or self.g_fwd), self.g_bwd)


# ---------------------------------------------------------------- DDPM inversion (reference modules/inverse_schedulers/ddpm_inverse_scheduler.py, modules/inversion/ddpm_inversion.py)
def ddpm_timesteps(S):
    """the scheduler's S leading-spaced timesteps, descending: the index order of the noised latents `xts` (index 0 = the largest t)"""
    return (np.arange(S) * (NUM_TRAIN // S))[::-1].astype(np.int64).copy()


def ddpm_alpha_prev(ac, final, S, t):
    p = int(t) - NUM_TRAIN // S
    return float(ac[p]) if p >= 0 else float(final)


def ddpm_variance(ac, final, S, t):
    """get_variance (:65-84) in float64 on the fp32 table"""
    a_t, a_p = float(ac[int(t)]), ddpm_alpha_prev(ac, final, S, t)
    return (1 - a_p) / (1 - a_t) * (1 - a_t / a_p)


def ddpm_sample_coefficients(ac, S, markovian, timesteps=None):
    """float64 [S][2] = (a, b) of etainv_ddpm_sample_latents per step in draw order (ascending t): from x_0, a = sqrt(abar_t), b = sqrt(1 - abar_t)
    (:118); Markovian, a = sqrt(abar_t / abar_prev), b = sqrt(1 - abar_t / abar_prev) with abar_prev = 1 below 0 (:121-124)"""
    ts = ddpm_timesteps(S)[::-1] if timesteps is None else [int(t) for t in timesteps]
    out = np.empty((len(ts), 2), dtype=np.float64)
    for s, t in enumerate(ts):
        p = int(t) - NUM_TRAIN // S
        q = float(ac[int(t)]) / (float(ac[p]) if p >= 0 else 1.0) if markovian else float(ac[int(t)])
        out[s] = q ** 0.5, (1 - q) ** 0.5
    return out


def ddpm_step_coefficients(ac, final, S, t):
    """float64 [5] of etainv_ddpm_invert_steps at timestep t (:169-193 with eta = 1): sqrt(1 - abar_t), sqrt(abar_t), sqrt(abar_prev),
    sqrt(1 - abar_prev - var), sigma = sqrt(var)"""
    a_t, a_p, var = float(ac[int(t)]), ddpm_alpha_prev(ac, final, S, t), ddpm_variance(ac, final, S, t)
    return np.array([(1 - a_t) ** 0.5, a_t ** 0.5, a_p ** 0.5, max(1 - a_p - var, 0.0) ** 0.5, var ** 0.5], dtype=np.float64)


def _f32c(t, what):
    if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
        raise ValueError(f"{what} must be a contiguous fp32 tensor, got {t.dtype}, contiguous {t.is_contiguous()}")
    return _capi.ptr(t)


def ddpm_sample_latents(lib, x0, noise, ab, markovian, stream=None):
    """etainv_ddpm_sample_latents: x0 (B,4,L,L), noise (S,B,4,L,L), ab float64 [S][2] -> xts (S+1,B,4,L,L)"""
    S, B, L = noise.shape[0], x0.shape[0], x0.shape[-1]
    if tuple(noise.shape) != (S, B, 4, L, L) or tuple(x0.shape) != (B, 4, L, L):
        raise ValueError(f"x0 (B,4,L,L) and noise (S,B,4,L,L) do not fit: {tuple(x0.shape)}, {tuple(noise.shape)}")
    ab = np.ascontiguousarray(ab, dtype=np.float64)
    assert ab.shape == (S, 2)
    xts = torch.empty(S + 1, B, 4, L, L, dtype=torch.float32, device=x0.device)
    _capi.check(lib.etainv_ddpm_sample_latents(_f32c(x0, "x0"), _f32c(noise, "noise"), ab.ctypes.data, int(bool(markovian)), _capi.ptr(xts), S, B, L,
                                               stream if stream is not None else _capi.stream_ptr()))
    return xts


def ddpm_invert_steps(lib, xts, first, k, eps_u, eps_c, g, coef, z, x_out, eps_out, stream=None):
    """etainv_ddpm_invert_steps on xts (S+1,B,4,L,L); eps_u (None: eps_c is the noise), eps_c, z, x_out, eps_out (None: not wanted) (k,B,4,L,L);
    coef float64 [k][5]"""
    S, B, L = xts.shape[0] - 1, xts.shape[1], xts.shape[-1]
    coef = np.ascontiguousarray(coef, dtype=np.float64)
    assert coef.shape == (k, 5)
    for name, t in (("eps_u", eps_u), ("eps_c", eps_c), ("z", z), ("x_out", x_out), ("eps_out", eps_out)):
        if t is not None and t.numel() != k * B * 4 * L * L:
            raise ValueError(f"{name} must hold {k} steps of {B} latents of side {L}, got {tuple(t.shape)}")
    _capi.check(lib.etainv_ddpm_invert_steps(_f32c(xts, "xts"), S, int(first), int(k), _f32c(eps_u, "eps_u"), _f32c(eps_c, "eps_c"), float(g),
                                             coef.ctypes.data, _f32c(z, "z"), _f32c(x_out, "x_out"), _f32c(eps_out, "eps_out"), B, L,
                                             stream if stream is not None else _capi.stream_ptr()))


def ddpm_backward_step(lib, x, eps_u, eps_c, scales, z, a_t, a_p, var, out_x, out_eps, stream=None):
    """etainv_ddpm_backward_step: x, eps_u, eps_c, out_x, out_eps (None: not wanted) (P B,4,L,L) rows [p0 x B, p1 x B, ..]; scales: P floats; z (B,4,L,L)"""
    P, B, L = len(scales), z.shape[0], z.shape[-1]
    for name, t in (("x", x), ("eps_u", eps_u), ("eps_c", eps_c), ("out_x", out_x), ("out_eps", out_eps)):
        if t is not None and tuple(t.shape) != (P * B, 4, L, L):
            raise ValueError(f"{name} must be ({P * B}, 4, {L}, {L}) = {P} prompt rows of {B} image(s), got {tuple(t.shape)}")
    g = np.ascontiguousarray(scales, dtype=np.float32)
    _capi.check(lib.etainv_ddpm_backward_step(_f32c(x, "x"), _f32c(eps_u, "eps_u"), _f32c(eps_c, "eps_c"), g.ctypes.data, P, _f32c(z, "z"), float(a_t),
                                              float(a_p), float(var), _f32c(out_x, "out_x"), _f32c(out_eps, "out_eps"), B, L,
                                              stream if stream is not None else _capi.stream_ptr()))


class DdpmLoop:
    """Edit-friendly DDPM inversion for B images at once.  `invert` is time-parallel: the noised latents of all steps come from one launch, so the
    S steps' noise predictions are ceil(rows / max_unet_batch) UNet calls with one timestep per row, each followed by one
    etainv_ddpm_invert_steps launch.  `sample` is sequential: per step one UNet call and one etainv_ddpm_backward_step launch.
    Tensors indexed by step follow `xts`: index j belongs to timestep t_bwd[j] (index 0 = the largest t)."""

    def __init__(self, engine, S=50, guidance_scale_fwd=3.5, guidance_scale_bwd=9.0, skip_steps=0.36, markovian_forward=False):
        self.e, self.S, self.L, self.lib = engine, int(S), engine.L, engine.lib
        self.g_fwd, self.g_bwd, self.markovian = float(guidance_scale_fwd), float(guidance_scale_bwd), bool(markovian_forward)
        self.skip = int(skip_steps * self.S)                       # backward steps skipped (get_bwd_skip, ddpm_inversion.py:120-126); 0 skips nothing
        ac = alphas_cumprod()
        self.t_bwd = ddpm_timesteps(self.S)
        self.ab = ddpm_sample_coefficients(ac, self.S, self.markovian)
        self.coef = np.stack([ddpm_step_coefficients(ac, ac[0], self.S, t) for t in self.t_bwd])
        self.bwd = [(float(ac[t]), ddpm_alpha_prev(ac, ac[0], self.S, t), ddpm_variance(ac, ac[0], self.S, t)) for t in self.t_bwd]
        self.rows_executed = self.unet_calls = 0

    def invert(self, z0, ctx_src, noise, guidance_scale_fwd=None):
        """z0 (B,4,L,L) fp32; ctx_src (B,2,77,768) = [uncond, cond] per image; noise (S,B,4,L,L), the draws of sample_latents in ascending t.
        Returns xts (S+1,B,4,L,L) and, per step in xts order, zs (the noise maps; the t = 0 one zeroed, ddpm_inversion.py:101), latents (the
        corrected x_{t-1}) and noise_preds, each (S,B,4,L,L)."""
        e, S, L = self.e, self.S, self.L
        g = self.g_fwd if guidance_scale_fwd is None else float(guidance_scale_fwd)
        guided = ddpm_guided(g)
        B, dev = z0.shape[0], z0.device
        xts = ddpm_sample_latents(self.lib, z0.float().contiguous(), noise.float().contiguous(), self.ab, self.markovian)
        zs, lat, eps = (torch.empty(S, B, 4, L, L, dtype=torch.float32, device=dev) for _ in range(3))
        ctx_u, ctx_c = ctx_src[:, 0].float(), ctx_src[:, 1].float()
        for ch in plan_ddpm_chunks(S, e.max_unet_batch, guided, B):
            sl = slice(ch.first, ch.first + ch.k)
            halves = [ctx_u, ctx_c] if guided else [ctx_c if g == 1.0 else ctx_u]
            ctx = torch.cat([h.repeat(ch.k, 1, 1) for h in halves]).contiguous()       # rows [u x k B, c x k B], a step's images side by side
            t_rows = [int(t) for t in self.t_bwd[sl] for _ in range(B)] * len(halves)   # equal timesteps at distance k B: the halves of a step
            out = e.unet(xts[sl].reshape(ch.k * B, 4, L, L), t_rows, ctx)
            eps_u, eps_c = (out[:ch.k * B], out[ch.k * B:]) if guided else (None, out)
            ddpm_invert_steps(self.lib, xts, ch.first, ch.k, eps_u, eps_c, g, self.coef[sl], zs[sl], lat[sl], eps[sl])
            self.rows_executed += ch.rows
            self.unet_calls += 1
        zs[S - 1].zero_()
        return {"xts": xts, "zs": zs, "latents": lat, "noise_preds": eps}

    def sample(self, inv, ctx_list, scales=None):
        """inv: result of `invert`; ctx_list: one (B,2,77,768) context per prompt -- [src, tgt] gives UNet rows [u_src x B, u_tgt x B, c_src x B,
        c_tgt x B] over the latents [src x B, tgt x B].  scales: one guidance scale per prompt (default: [g_fwd, g_bwd] for two prompts, g_bwd
        otherwise, ddpm_inversion.py:154-159).  Returns the final latents (n B, 4, L, L)."""
        skip = self.skip
        start = inv["latents"][skip - 1] if skip > 0 else inv["xts"][0]
        ctx = torch.cat([torch.cat([c[:, 0] for c in ctx_list]), torch.cat([c[:, 1] for c in ctx_list])])
        return self.backward(torch.cat([start] * len(ctx_list)), ctx, [inv["zs"][j] for j in range(skip, self.S)], scales)

    def backward(self, x, ctx, zs, scales=None):
        """the last len(zs) backward steps from x (n B,4,L,L), rows [p0 x B, p1 x B, ..], under ctx (2 n B,77,768), rows [uncond x n B, cond x n B];
        zs: the noise map (B,4,L,L) of every step"""
        e, L, S = self.e, self.L, self.S
        B = zs[0].shape[0]
        n_p = x.shape[0] // B
        if x.shape[0] != n_p * B or ctx.shape[0] != 2 * n_p * B or len(zs) > S:
            raise ValueError(f"{x.shape[0]} latents, {ctx.shape[0]} context rows, {B} image(s) and {len(zs)} steps of {S} do not fit")
        if scales is None:
            scales = [self.g_fwd, self.g_bwd] if n_p == 2 else [self.g_bwd] * n_p
        x, ctx = x.float().contiguous().clone(), ctx.float().contiguous()
        x_next, eps_all = torch.empty_like(x), torch.empty(2 * n_p * B, 4, L, L, dtype=torch.float32, device=x.device)
        with e.cached_context():
            for j, z in zip(range(S - len(zs), S), zs):
                e.unet(x, int(self.t_bwd[j]), ctx, None, out=eps_all)
                a_t, a_p, var = self.bwd[j]
                ddpm_backward_step(self.lib, x, eps_all[:n_p * B], eps_all[n_p * B:], scales, z.float().contiguous(), a_t, a_p, var, x_next, None)
                x, x_next = x_next, x
                self.rows_executed += 2 * n_p * B
                self.unet_calls += 1
        return x

    def expected_rows(self, B, n_prompts, guidance_scale_fwd=None):
        """UNet sample-forwards of one invert + one sample (flops.ddpm_unet_rows)"""
        return ddpm_unet_rows(self.S, self.skip, B, n_prompts, self.g_fwd if guidance_scale_fwd is None else float(guidance_scale_fwd))
