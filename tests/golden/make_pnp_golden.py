#!/usr/bin/env python3
"""Generate the plug-and-play fixtures of tests/golden.

    cd /tmp && python <repo>/tests/golden/make_pnp_golden.py --reference     # pnp_schedule.npz, e2e_pnp.npz
    cd /tmp && python <repo>/tests/golden/make_pnp_golden.py --oracle        # pnp_sd.npz

--reference RUNS THE REFERENCE'S OWN CODE (modules/editing/pnp_editor.py PlugAndPlayEditor, modules/utils/pnp.py register_pnp / PnPUnetForward,
modules/utils/pnp_utils.py register_time and the two hook installers) with the import stubs, fake pipeline and toy-width UNet of make_golden.py,
so it needs the reference checkout that script names.  On top of those stubs it needs a `UNet2DConditionOutput` that answers ["sample"], a
tokenizer that takes a bare string (get_text_embeds passes one), and on the hooked residual block the attributes of the diffusers module that
the reference's forward reads and the oracle's module does not carry (as make_golden.gen_resnet_block sets them).  Everything runs under
torch.no_grad().

--oracle needs only this repository: tests/pnp_ref.py (pinned against the --reference fixtures by tests/test_pnp_ref.py) over the SD-width
oracle UNet in float64 at 16 x 16 latents, two images per call -- the expected values of the GPU tests (tests/test_pnp_gpu.py)."""
import argparse
import sys
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

HERE = Path(__file__).resolve().parent
REPO = HERE.parents[1]
sys.path.insert(0, str(REPO))

SCHEDULE_S = (3, 5, 50)
E2E_S = 5
ETA = [[0.6, 0], [1, 0.7]]


class UNet2DConditionOutput(dict):
    def __init__(self, sample):
        super().__init__(sample=sample)
        self.sample = sample


def install_pnp_stubs(mg):
    from tests.golden.make_edict_golden import install_edict_stubs
    install_edict_stubs(mg)                                     # (the reference's pnp editor imports its edict inverter)
    sys.modules["diffusers.models.unet_2d_condition"].UNet2DConditionOutput = UNet2DConditionOutput


def make_pipe(mg, unet):
    pipe = mg.make_pipe(unet)
    tok = pipe.tokenizer
    pipe.tokenizer = lambda texts, **k: tok([texts] if isinstance(texts, str) else texts, **k)
    pipe.tokenizer.model_max_length = tok.model_max_length
    pipe.tokenizer.decode, pipe.tokenizer.encode = tok.decode, tok.encode
    blk = unet.up_blocks[1].resnets[1]
    blk.nonlinearity, blk.upsample, blk.downsample = F.silu, None, None
    blk.time_embedding_norm, blk.output_scale_factor, blk.dropout = "default", 1.0, torch.nn.Identity()
    return pipe


def hooked_modules(unet):
    from tests.pnp_ref import QK_SITES
    return unet.up_blocks[1].resnets[1], [unet.up_blocks[i].attentions[j].transformer_blocks[0].attn1 for i, js in QK_SITES.items() for j in js]


def fires(mod):
    """the hooked module's own condition (pnp_utils.py:81-82, 173) on the state register_time / the installers left on it"""
    return bool(mod.injection_schedule is not None and (mod.t in mod.injection_schedule or mod.t == 1000))


def gen_schedule(mg):
    """per S and backward step: t, whether the conv hook fires, whether the Q/K hooks fire -- read off the reference's hooked modules after its own
    register_pnp (windows from model.scheduler) and register_time; no UNet call needed"""
    from modules.inversion.eta_inversion import EtaInversion
    from modules.utils.pnp import register_pnp, unregister_pnp
    from modules.utils.pnp_utils import register_time
    out = {}
    unet = mg.toy_unet(0)
    for S in SCHEDULE_S:
        pipe = make_pipe(mg, unet)
        EtaInversion(pipe, scheduler="ddim", num_inference_steps=S)                 # sets pipe.scheduler to the backward scheduler with S timesteps
        register_pnp(pipe, None)
        conv_mod, attn_mods = hooked_modules(unet)
        rows = []
        for t in pipe.scheduler.timesteps:
            register_time(pipe, t.item())
            qk = {fires(m) for m in attn_mods}
            assert len(qk) == 1
            rows.append([int(t), int(fires(conv_mod)), int(qk.pop())])
        unregister_pnp(pipe)
        out[f"S{S}"] = np.array(rows, dtype=np.int64)
    mg.save("pnp_schedule", **out)


def gen_e2e(mg, S=E2E_S):
    """the reference's PlugAndPlayEditor over etainv and dirinv on the toy UNet, with a per-call record of what the hooked modules did"""
    from modules.inversion.eta_inversion import EtaInversion
    from modules.inversion.direct_inversion import DirectInversion
    from modules.editing.pnp_editor import PlugAndPlayEditor
    src, tgt = mg.PROMPT_PAIRS[0]
    unet = mg.toy_unet(0)
    z0 = 0.8 * torch.randn(1, 4, 64, 64, generator=torch.Generator().manual_seed(2033))
    out = {"z0": z0, "S": np.array(S)}
    for tag in ("etainv", "dirinv"):
        pipe = make_pipe(mg, unet)
        if tag == "etainv":
            inv = EtaInversion(pipe, scheduler="ddim", num_inference_steps=S, eta=ETA, noise_sample_count=10, seed=0)
        else:
            inv = DirectInversion(pipe, scheduler="ddim", num_inference_steps=S)
        captured, calls = {}, []
        orig_inv, orig_step = inv.invert, inv.predict_step_backward

        def wrapped_inv(*a, _o=orig_inv, **k):
            captured["inv"] = _o(*a, **k)
            return captured["inv"]

        def wrapped_step(latent, t, *a, _o=orig_step, **k):
            new, eps = _o(latent, t, *a, **k)
            conv_mod, attn_mods = hooked_modules(unet)
            calls.append([int(t), int(fires(conv_mod)), int(fires(attn_mods[0])), int(unet.forward.idx)])
            return new, eps
        inv.invert, inv.predict_step_backward = wrapped_inv, wrapped_step
        ed = PlugAndPlayEditor(inv)
        res = ed.edit(z0 / 0.18215, src, tgt, inv_cfg=dict(edit_word_idx=(1, 1)))
        out[f"{tag}/latent_inv"], out[f"{tag}/latent"] = res["latent_inv"], res["latent"]
        out[f"{tag}/calls"] = np.array(calls, dtype=np.int64)                        # t, conv fired, qk fired, PnPUnetForward call count
        if tag == "etainv":
            out["zT_inv"] = captured["inv"]["latents"][-1]                           # (the trajectory itself is pinned by e2e_toy / e2e_dirinv)
    # the contexts are regenerated by the test from make_golden's stand-in text encoder; stored as a probe (1 MiB per fixture)
    ctx_s, ctx_t = captured["inv"]["context"], inv.create_context(tgt, negative_prompt=ed.negative_prompt)
    out["ctx_probe"] = torch.cat([ctx_s.flatten()[:4], ctx_s.flatten()[-4:], ctx_t.flatten()[:4], ctx_t.flatten()[-4:]])
    mg.save("e2e_pnp", **out)


def gen_sd():
    from oracle.unet import build_unet
    from oracle import loop as oloop
    from tests import pnp_ref as pr
    # float64 arithmetic on the fp32 inputs and weights, results stored as fp32: the GPU tests hold the fp32-operand engine to atol 1e-4 after five
    # guided steps, and an fp32 CPU run is itself up to 1.2e-4 away from this one on these inputs (summation order through the 7.5 x guidance) -- a
    # reference has to be well inside the bound it is used with
    unet = build_unet(0).double()
    S, L, n = pr.SD_S, pr.SD_L, pr.SD_N_IMG
    z0, ctx_src, ctx_tgt = pr.sd_case_inputs()
    lat, ctx, t = pr.sd_call_inputs()
    out = {"S": np.array(S), "probe": torch.cat([z0.flatten()[:4], ctx_src.flatten()[-4:], ctx_tgt.flatten()[:4], lat.flatten()[-4:]]).numpy()}
    z0, ctx_src, ctx_tgt, lat, ctx = (v.double() for v in (z0, ctx_src, ctx_tgt, lat, ctx))
    hooked = pr.PnpUNet(unet, n)
    with hooked.hooked():
        for tag, (conv, qk) in {"none": (False, False), "conv": (True, False), "qk": (False, True), "both": (True, True)}.items():
            hooked.conv_on, hooked.qk_on = conv, qk
            out[f"call/{tag}"] = hooked.rows3(lat, torch.tensor(t), ctx).numpy()
    assert hooked.fired == {"conv": 2, "qk": 16}
    noise = oloop.noise_table(S, 10, L, seed=0).double()
    for k in range(n):                                                             # the oracle's loop holds one image: one run per image
        o = oloop.EtaInversionOracle(unet, S=S, eta=pr.ETA, L=L, use_mask=False, dtype=torch.float64)
        inv = o.invert(z0[k:k + 1], ctx_src[k], "x")
        trace = []
        z = pr.pnp_sample_ref(o, inv, ctx_src[k], ctx_tgt[k], noise, trace=trace)
        out[f"loop/{k}/inv_latents"] = torch.cat(inv["latents"]).numpy()
        out[f"loop/{k}/latent"] = z.numpy()
        out[f"loop/{k}/bwd_latents"] = torch.stack([e["latent"] for e in trace]).numpy()
        out[f"loop/{k}/eps_rows"] = torch.stack([e["eps_rows"] for e in trace]).numpy()     # [u_s, u_t, c_t] per step
        out[f"loop/{k}/best"] = np.array([e["best"] for e in trace])
        out[f"loop/{k}/flags"] = np.array([[int(e["conv"]), int(e["qk"])] for e in trace])
    # dirinv + pnp on image 0: the eta = 0, mask-free loop (every step replays the source row; the last step runs neither injection)
    o = oloop.EtaInversionOracle(unet, S=S, eta=(0.0, 0.0), noise_sample_count=1, L=L, use_mask=False, dtype=torch.float64)
    inv = o.invert(z0[:1], ctx_src[0], "x")
    out["dirinv/latent"] = pr.pnp_sample_ref(o, inv, ctx_src[0], ctx_tgt[0], oloop.noise_table(S, 1, L, seed=0).double()).numpy()
    out = {k: v.astype(np.float32) if v.dtype == np.float64 else v for k, v in out.items()}
    np.savez_compressed(HERE / "pnp_sd.npz", **out)
    print("wrote pnp_sd.npz:", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--oracle", action="store_true")
    ap.add_argument("--only", default=None, choices=("schedule", "e2e"))
    a = ap.parse_args()
    assert Path.cwd() != REPO, "run from a scratch directory (the reference removes result folders at import time)"
    torch.set_grad_enabled(False)
    if a.reference:
        from tests.golden import make_golden as mg
        install_pnp_stubs(mg)
        with torch.no_grad():
            if a.only in (None, "schedule"):
                gen_schedule(mg)
            if a.only in (None, "e2e"):
                gen_e2e(mg)
    if a.oracle:
        gen_sd()
