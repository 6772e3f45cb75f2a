"""The backward pass of `etainv.pipeline.EtaLoop.sample` as data: which UNet rows run at every step and what the step does with their noise.
It depends on host scalars only (eta table, the controllers' step windows, A/B switches): decided before the loop, which executes record by record."""
from collections import namedtuple

from .flops import exit_share

# One UNet call.  A role is a context row group of B rows (u / c: uncond / cond prompt, s / t: source / target); UNet row group r reads latent group
# r % len(latents) (the engine's rule), so every role must meet a latent of its own side.  eu / ec: the groups whose noise is the target's guidance
# pair; n_out: the leading groups with an output (a source row that leaves the network early has none); ctrl: whether the attention control is passed.
Layout = namedtuple("Layout", "roles latents eu ec n_out ctrl")
FULL, PNP = "u_s,u_t,c_s,c_t", "u_s,u_t,c_t"
LAYOUTS = {
    FULL:          Layout(("u_s", "u_t", "c_s", "c_t"), ("src", "tgt"), 1, 3, 4, True),          # the reference's call
    "u_t,c_s,c_t": Layout(("u_t", "c_s", "c_t"), ("tgt", "src"), 0, 2, 3, True),                 # ptp, source replayed: c_s stays, its probabilities are injected
    "u_t,c_t,c_s": Layout(("u_t", "c_t", "c_s"), ("tgt", "tgt", "src"), 0, 1, 2, True),          # ... and c_s leaves after src_exit_block: it only feeds the map store
    PNP:           Layout(("u_s", "u_t", "c_t"), ("src", "tgt", "tgt"), 1, 2, 3, True),          # plug-and-play cuts c_s (pnp.py:130-146)
    "u_t,c_t":     Layout(("u_t", "c_t"), ("tgt",), 0, 1, 2, False),                             # nothing reads the source rows
}

# (a_t, a_p, var): the DDIM-eta coefficients; replay: the source row is copied from the inversion trajectory and the target takes a plain DDIM
# step; layout / trace_layout: what runs / what the trace reports (the rows with an output); first_row .. pnp_conv_active: the attention
# control (edit: cross edit live); blend: LocalBlend after the step; cost: UNet sample-forwards per image, from the layout's rows
Step = namedtuple("Step", "t a_t a_p var eta replay layout trace_layout first_row src_exit_block edit self_replace_active masa_active "
                          "pnp_qk_active pnp_conv_active blend cost")


def plan_backward(S, t_bwd, etas, ac, delta, L, B=1, skip_dead_source_rows=True, src_exit=True, src_exit_9_only=False, ptp=None, masactrl=None, pnp=None):
    """One Step per backward timestep.  ac: float64 alphas_cumprod; ptp: anything with cross_active, self_lo, self_hi and blend_alpha (None or
    not); masactrl: (start_step, first_block); pnp: (conv_steps, qk_steps); at most one of the three."""
    steps, pnp, ts = [], pnp and (int(pnp[0]), int(pnp[1])), [int(t) for t in t_bwd]
    tables = ts, ac[ts].tolist(), ac[[max(t - delta, 0) for t in ts]].tolist(), etas[ts].tolist()   # (below the last timestep: alphas_cumprod[0])
    for i, (t, a_t, a_p, eta) in enumerate(zip(*tables)):
        var = (1 - a_p) / (1 - a_t) * (1 - a_t / a_p)                                       # (float64 Python arithmetic on the float64 table)
        replay = bool(skip_dead_source_rows) and eta == 0.0 and masactrl is None           # (MasaCtrl couples u_t to u_s: all four rows stay)
        edit = ptp is not None and bool(ptp.cross_active[i])
        self_on = ptp is not None and ptp.self_lo <= i < ptp.self_hi
        first_row = exit_block = 0
        if pnp is not None:         # while an injection is live the target rows read the u_s row inside the network: it runs although its noise is unused
            layout = "u_t,c_t" if replay and i >= max(pnp) else PNP
        elif not replay or ptp is None:
            layout = "u_t,c_t" if replay else FULL
        elif not edit and src_exit and not (src_exit_9_only and self_on):
            # no cross replacement any more: c_s only feeds the AttentionStore of the five (L/4)^2 cross layers (LocalBlend / bwd_* masks; last one
            # = block 9) and, while the self-replace runs, the (L/2)^2-token self-attentions (last one = block 12)
            layout, first_row, exit_block = "u_t,c_t,c_s", B, 12 if self_on else 9
        else:
            layout, first_row = "u_t,c_s,c_t", B
        cost = LAYOUTS[layout].n_out + (exit_share(L, exit_block) if exit_block else 0.0)    # an exited row: the share of the FLOPs it ran
        steps.append(Step(t, a_t, a_p, var, eta, replay, layout, "u_t,c_t" if exit_block else layout, first_row, exit_block, edit, self_on,
                          masactrl is not None and masactrl[0] <= i < 50,                  # (50: the reference's own window, whatever S is)
                          pnp is not None and i < pnp[1], pnp is not None and i < pnp[0],
                          ptp is not None and ptp.blend_alpha is not None and (i + 1) > int(0.2 * S), cost))
    return steps


# ---- time-parallel DDPM inversion (etainv.pipeline.DdpmLoop.invert, modules/inversion/ddpm_inversion.py): all noised latents exist before the first
# UNet call, so the S steps go to the UNet in chunks of whole steps.  first / k: the chunk's steps, as indices into xts (index 0 = the largest t);
# rows: its UNet rows, [u x k n_img, c x k n_img] when guided, [one half x k n_img] otherwise
Chunk = namedtuple("Chunk", "first k rows")
DDPM_MAX_CHUNK = 128                                    # steps per etainv_ddpm_invert_steps launch (ETAINV_DDPM_MAX_CHUNK)


def ddpm_guided(g):
    """predict_noise runs both halves of a step unless the scale is 0 or 1 (reference diffusion_inversion.py:263-286)"""
    return float(g) not in (0.0, 1.0)


def plan_ddpm_chunks(S, max_rows, guided, n_img=1):
    """Chunks that cover the steps 0 .. S-1 once, in order, each of at most max_rows UNet rows.  The two halves of a step stay in one call."""
    per_step = int(n_img) * (2 if guided else 1)
    if S < 1 or n_img < 1:
        raise ValueError(f"S and n_img must be at least 1, got {S} and {n_img}")
    if per_step > max_rows:
        raise ValueError(f"one step of {n_img} image(s) is {per_step} UNet rows, the engine takes {max_rows} per call")
    k = min(max_rows // per_step, DDPM_MAX_CHUNK)
    return [Chunk(first, min(k, S - first), min(k, S - first) * per_step) for first in range(0, S, k)]
