"""Plug-and-Play editor (reference modules/editing/pnp_editor.py:12-71 with modules/utils/pnp.py:86-150 and modules/utils/pnp_utils.py:44-195):
during the backward pass the UNet runs rows [u_s, u_t, c_t] -- the cond source row is cut and the uncond source noise returned in its place -- and
the target rows take, from the u_s row, the conv2 output of up_blocks[1].resnets[1] for the first int(S * 0.8) steps and Q, K of the self-attention
of transformer blocks 8..15 for the first int(S * 0.5) steps.  The target's uncond row is the negative prompt below."""
from .controller import ControllerBase
from .editor import Editor, _split

NEGATIVE_PROMPT = "ugly, blurry, black, low res, unrealistic"


def injection_steps(num_inference_steps: int, pnp_f_t: float = 0.8, pnp_attn_t: float = 0.5):
    """(conv_steps, qk_steps): the number of leading backward steps with the feature / the Q,K injection -- `scheduler.timesteps[:int(S * f)]`
    of init_pnp (pnp.py:50-54, 91-92)"""
    return int(num_inference_steps * pnp_f_t), int(num_inference_steps * pnp_attn_t)


class PnpController(ControllerBase):
    def __init__(self, conv_steps: int, qk_steps: int, model=None):
        self.conv_steps, self.qk_steps, self.model, self.step_idx = conv_steps, qk_steps, model, 0

    # per-step API (the batched device loop reads conv_steps / qk_steps directly): hand this step's declarative control to model.unet
    def begin(self) -> None:
        self.step_idx = 0

    def end(self) -> None:
        if self.model is not None:
            self.model.unet.attn_ctrl = None

    def begin_step(self, latent, *args, **kwargs):
        if self.model is not None:
            from etainv import _capi
            from etainv.engine import AttnControl
            self.model.unet.attn_ctrl = AttnControl(mode=_capi.ATTN_PNP, n_img=1, pnp_qk_active=self.step_idx < self.qk_steps,
                                                    pnp_conv_active=self.step_idx < self.conv_steps)
        return latent

    def end_step(self, latent, noise_pred=None, t=None):
        if self.model is not None:
            self.model.unet.attn_ctrl = None
        self.step_idx += 1
        return latent


class PlugAndPlayEditor(Editor):
    def __init__(self, inverter, no_null_source_prompt: bool = True) -> None:
        from ..inversion.diffusion_inversion import DiffusionInversion
        from ..inversion.direct_inversion import DirectInversion
        from ..inversion.eta_inversion import EtaInversion
        # the injections couple the rows of ONE UNet call per step; an EDICT pair would need them per pair member (two calls per step, each with its
        # own source row), which is not built
        if type(inverter) not in (DiffusionInversion, EtaInversion, DirectInversion):
            raise NotImplementedError(f"the pnp editor is built for the etainv, dirinv and diffinv inverters (one [source, target] UNet call per backward "
                                      f"step), got {type(inverter).__name__}")
        self.inverter, self.model = inverter, inverter.model
        self.negative_prompt = NEGATIVE_PROMPT
        self.no_null_source_prompt = no_null_source_prompt

    def edit(self, image, source_prompt, target_prompt, cfg=None, inv_cfg=None):
        assert cfg is None, f"{cfg}"
        inv_cfg = {} if inv_cfg is None else inv_cfg
        src_context = self.inverter.create_context("" if not self.no_null_source_prompt else source_prompt)
        target_context = self.inverter.create_context(target_prompt, negative_prompt=self.negative_prompt or "")
        inv_res = self.inverter.invert(image, prompt=source_prompt, context=src_context, inv_cfg=inv_cfg)
        conv_steps, qk_steps = injection_steps(self.inverter.num_inference_steps)
        with self.inverter.use_controller(PnpController(conv_steps, qk_steps, self.model)):
            edit_res = self.inverter.sample(inv_res, context=[src_context, target_context])
        return None if edit_res is None else _split(edit_res)
