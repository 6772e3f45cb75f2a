"""The `npi` and `proxnpi` inverters on the engine: plugin + simple editor against tests/golden/npi_sd.npz (tests/proxnpi_ref.py over the
SD-width oracle UNet in float64, 16 x 16 latents, S = 3), fused path == per-step path, the guidance-1 case, prompt-to-prompt and MasaCtrl
through the per-step backward pass, the `invedit` editor, and the command line.

Bounds.  fp32 pipeline: the project's 1e-3 relative L2 on inversion and edited latents, and on the thresholds.  fp16 pipeline: `npi` holds
the project's 3e-2 on edited latents; `proxnpi` (l0) may be at most 3 x the npi run's measured error -- the shrinkage is 1-Lipschitz in d and
the threshold moves by no more than the largest input error, so the 3 is room for an operation applied to the 16-bit UNet's noise, as in
tests/test_regdiff_gpu.py.  `proxnpi` (l1) is checked in the fp32 pipeline only: its two jumps (the fixture's l1_margins) are further from
every |d| than fp32 moves them, not than fp16 does.

Measured on MI355X (this file's own printouts): see DESIGN.md, "Proximal guidance"."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import edict_ref as er

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
SRC, TGT = "a cat sitting next to a mirror", "a tiger sitting next to a mirror"
L, S = er.SD_L, er.SD_S


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return ((a - b).norm() / b.norm()).item()


@pytest.fixture(scope="module")
def case():
    z0, ctx_s, ctx_t = er.sd_case_inputs()
    g = np.load(ROOT / "tests" / "golden" / "npi_sd.npz")
    assert int(g["S"]) == S
    np.testing.assert_array_equal(np.concatenate([z0.ravel()[:4], ctx_s.ravel()[:4], ctx_t.ravel()[:4]]), g["probe"])
    f = lambda v: torch.from_numpy(v).float().cuda()
    return dict(z0=f(z0), ctx={SRC: f(ctx_s), TGT: f(ctx_t)}, g=g)


@pytest.fixture(scope="module")
def pipes():
    """variant -> pipeline, built on first use, one each for the whole module"""
    import modules
    made = {}

    def get(variant):
        if variant not in made:
            made[variant] = modules.load_diffusion_model("sd15", "cuda", variant=variant, latent_size=L, max_img=3)[0]
        return made[variant]
    yield get
    for p in made.values():
        p.engine.close()


def _inverter(p, case, name="npi", **kw):
    """the inverter fed with the case's latent and contexts directly (the VAE and the text encoder are tested elsewhere)"""
    import modules
    inv = modules.load_inverter(name, model=p, scheduler="ddim", num_inference_steps=S, **kw)
    inv.encode = lambda image: image.to("cuda").float()
    inv.create_context = lambda prompt, negative_prompt="": case["ctx"][prompt]
    return inv


def _record_thresholds(inv):
    """wrap the inverter's one kernel call: every launch also returns its (thr, v_k, v_k+1)"""
    seen, orig = [], inv._guide

    def guide(eps_u, eps_c, g, x=None, a_from=1.0, a_to=1.0, thr_out=None):
        thr_out = torch.zeros(1, 3, device="cuda")
        res = orig(eps_u, eps_c, g, x, a_from, a_to, thr_out=thr_out)
        seen.append(thr_out.cpu())
        return res
    inv._guide = guide
    return seen


def _edit_vs_oracle(p, case, tag, variant):
    """invert + simple edit of one variant; returns (inversion error, source error, target error, thresholds of the backward launches)"""
    import modules
    g = case["g"]
    kw = {} if tag == "npi" else dict(prox=tag[-2:], quantile=float(g[f"{tag}/quantile"]))
    inv = _inverter(p, case, tag.split("_")[0], **kw)
    thrs = _record_thresholds(inv)
    res = inv.invert(case["z0"], prompt=SRC, context=case["ctx"][SRC])
    assert {"latents", "noise_preds", "zT_inv", "context", "uncond_embeddings"} <= set(res) and len(res["latents"]) == S + 1
    assert len(res["uncond_embeddings"]) == S and torch.equal(res["uncond_embeddings"][0], case["ctx"][SRC][1:2])
    e_inv = rel(torch.stack(res["latents"]), g["inv_latents"])
    edit = modules.load_editor("simple", inverter=inv).edit(case["z0"], SRC, TGT)
    assert set(edit) == {"image_inv", "image", "latent_inv", "latent"} and edit["image"].shape == (1, 3, 8 * L, 8 * L)
    assert len(thrs) == S                                                           # the fused path: one launch per backward step
    e_s, e_t = rel(edit["latent_inv"], g[f"{tag}/edit"][0:1]), rel(edit["latent"], g[f"{tag}/edit"][1:2])
    print(f"{tag} + simple vs oracle ({variant}): inversion rel L2 {e_inv:.3e}, edited latents source {e_s:.3e}, target {e_t:.3e}")
    return e_inv, e_s, e_t, thrs


@pytest.mark.parametrize("tag", ["npi", "proxnpi_l0", "proxnpi_l1"])
def test_plugin_simple_vs_oracle_fp32(pipes, case, tag):
    g = case["g"]
    e_inv, e_s, e_t, thrs = _edit_vs_oracle(pipes("fp32"), case, tag, "fp32")
    assert e_inv < 1e-3 and e_s < 1e-3 and e_t < 1e-3
    if tag != "npi":
        got = torch.stack([t[0, 0] for t in thrs]).double().numpy()
        e_thr = np.abs(got / g[f"{tag}/thr"] - 1).max()
        print(f"{tag} thresholds {got} vs oracle {g[f'{tag}/thr']}: relative {e_thr:.3e}")
        assert e_thr < 1e-3
        assert (torch.stack([t[0, 1] for t in thrs]) > 0).all()                      # above the zeros of the source pair


def test_plugin_simple_vs_oracle_fp16(pipes, case):
    """npi at the project's fp16 bounds; proxnpi (l0) at no more than 3 x the npi run's measured error"""
    p = pipes("fp16")
    e_inv, e_s, e_t, _ = _edit_vs_oracle(p, case, "npi", "fp16")
    assert e_inv < 5e-3 and e_s < 3e-2 and e_t < 3e-2
    base = max(e_s, e_t)
    _, p_s, p_t, _ = _edit_vs_oracle(p, case, "proxnpi_l0", "fp16")
    print(f"proxnpi_l0 (fp16): error {max(p_s, p_t):.3e} = {max(p_s, p_t) / base:.2f} x the npi run's {base:.3e} (bound 3)")
    assert max(p_s, p_t) <= 3 * base


@pytest.mark.parametrize("name,kw", [("npi", {}), ("proxnpi", {}), ("proxnpi", dict(prox="l1", quantile=0.65))])
def test_fused_path_equals_per_step_path(pipes, case, name, kw):
    """the fused step (UNet, one launch) vs predict_step_backward (hooks, UNet, guidance launch, scheduler kernel): the hooks are called once
    per step and the results differ by contraction in the DDIM step only"""
    from modules.editing.controller import ControllerBase
    inv = _inverter(pipes("fp32"), case, name, **kw)
    res = inv.invert(case["z0"], context=case["ctx"][SRC])
    contexts = [case["ctx"][SRC], case["ctx"][TGT]]
    fast = inv.sample(res, context=contexts)["latent"]

    class Counting(ControllerBase):
        begun = ended = 0

        def begin_step(self, latent, *a, **k):
            self.begun += 1
            return latent

        def end_step(self, latent, noise_pred=None, t=None):
            assert noise_pred is not None and t is not None
            self.ended += 1
            return latent
    rec = Counting()
    inv.force_per_step = True
    with inv.use_controller(rec):
        slow = inv.sample(res, context=contexts)["latent"]
    forced = inv.sample(res, context=contexts)["latent"]                              # per-step path without a controller
    inv.force_per_step = False
    assert (rec.begun, rec.ended) == (S, S)
    e = rel(fast, slow)
    print(f"{name} {kw}: fused vs per-step path rel L2 {e:.3e}")
    assert e < 1e-5 and torch.equal(forced, slow)


def test_context_tensor_is_not_modified(pipes, case):
    """the reference writes the conditional embedding into the caller's context (a deviation, negative_prompt_inversion.py's docstring)"""
    inv = _inverter(pipes("fp32"), case, "npi")
    res = inv.invert(case["z0"], context=case["ctx"][SRC])
    ctx = case["ctx"][TGT].clone()
    for per_step in (False, True):
        inv.force_per_step = per_step
        out = inv.sample(res, context=ctx)
        assert torch.equal(ctx, case["ctx"][TGT]) and out["latent"].shape == (1, 4, L, L)
    # and what it computes under a single tensor is the target row's first unconditional row replaced, i.e. the pair [cond source, cond target]
    want = inv.sample(res, context=torch.stack([case["ctx"][SRC][1], case["ctx"][TGT][1]]))["latent"]
    assert torch.equal(out["latent"], want)


def test_guidance_one_takes_no_shortcut(pipes, case):
    """at guidance 1 the base class runs the cond half alone (eps = eps_c); proxnpi must run both halves: eps_u + d' is not eps_c"""
    g = case["g"]
    p = pipes("fp32")
    calls = []
    orig = p.unet.__class__.__call__

    def counted(self, sample, timestep, encoder_hidden_states=None):
        calls.append(sample.shape[0])
        return orig(self, sample, timestep, encoder_hidden_states)
    results = {}
    try:
        p.unet.__class__.__call__ = counted
        for name in ("npi", "proxnpi"):
            for per_step in (False, True):
                inv = _inverter(p, case, name, guidance_scale_bwd=1)
                res = {"latents": [torch.from_numpy(g["inv_latents"][-1]).float().cuda()], "uncond_embeddings": [case["ctx"][SRC][1:2]] * S}
                inv.force_per_step = per_step
                calls.clear()
                results[name, per_step] = inv.sample(res, context=[case["ctx"][SRC], case["ctx"][TGT]])["latent"]
                assert calls == ([2] * S if name == "npi" else [4] * S), (name, per_step, calls)
    finally:
        p.unet.__class__.__call__ = orig
    for per_step in (False, True):
        e_p, e_n = rel(results["proxnpi", per_step], g["proxnpi_l0_g1/edit"]), rel(results["npi", per_step], g["npi_g1/edit"])
        moved = rel(results["proxnpi", per_step][1:], results["npi", per_step][1:])
        print(f"guidance 1 (per_step {per_step}): proxnpi vs restatement {e_p:.3e}, npi {e_n:.3e}; proxnpi differs from npi by {moved:.3e} on the target")
        assert e_p < 1e-3 and e_n < 1e-3 and moved > 1e-2
    assert rel(results["proxnpi", False], results["proxnpi", True]) < 1e-5


def test_attention_editors_run_the_per_step_path(pipes, case):
    import modules
    p = pipes("fp32")
    npi, prox = _inverter(p, case, "npi"), _inverter(p, case, "proxnpi")
    simple = {id(inv): modules.load_editor("simple", inverter=inv).edit(case["z0"], SRC, TGT) for inv in (npi, prox)}
    ptp_cfg = dict(is_replace_controller=False, prompts=[SRC, TGT], cross_replace_steps={"default_": .4}, self_replace_steps=0.6,
                   equilizer_params={"words": ("tiger",), "values": (2,)})
    for inv, editor, cfg in ((npi, "ptp", ptp_cfg), (prox, "masactrl", None)):
        steps = []
        orig = inv.predict_step_backward

        def counted(latent, t, *a, _o=orig, **k):
            steps.append(int(t))
            return _o(latent, t, *a, **k)
        inv.predict_step_backward = counted
        # (MasaCtrl from the second of the three steps on, in transformer blocks >= 4: the reference's defaults, 4 and 10, are for 50 steps)
        ed = modules.load_editor(editor, inverter=inv) if cfg else modules.load_editor(editor, inverter=inv, step=1, layer=4)
        res = ed.edit(case["z0"], SRC, TGT, cfg={**cfg} if cfg else None)
        assert len(steps) == S and p.unet.attn_ctrl is None
        assert torch.isfinite(res["latent"]).all() and torch.isfinite(res["latent_inv"]).all()
        moved = rel(res["latent"], simple[id(inv)]["latent"])
        e_src = rel(res["latent_inv"], simple[id(inv)]["latent_inv"])
        print(f"{type(inv).__name__} + {editor}: target differs from simple by {moved:.3e}, source row by {e_src:.3e}")
        assert moved > 1e-3                                                            # the attention edit changes the target row
        if editor == "ptp":
            assert e_src < 1e-3                                                        # and leaves the source row alone


def test_invedit(pipes, case):
    import modules
    p = pipes("fp32")
    inv = _inverter(p, case, "npi")
    ed = modules.load_editor("invedit", inverter=inv)
    res = ed.edit(case["z0"], SRC, TGT)
    assert set(res) == {"image", "latent"} and res["latent"].shape == (1, 4, L, L) and res["image"].shape == (1, 3, 8 * L, 8 * L)
    e = rel(res["latent"], case["g"]["invedit"])
    print(f"invedit + npi vs oracle: reconstruction rel L2 {e:.3e}")
    assert e < 1e-3
    # vae_rec: the VAE round trip, no diffusion (the real encode / decode: an image in, an image out)
    real = modules.load_inverter("npi", model=p, scheduler="ddim", num_inference_steps=S)
    image = torch.rand(1, 3, 8 * L, 8 * L, generator=torch.Generator().manual_seed(3)).cuda() * 2 - 1
    rec = modules.load_editor("invedit", inverter=real, vae_rec=True).edit(image, SRC, TGT)
    assert set(rec) == {"image", "latent"} and torch.equal(rec["latent"], real.encode(image)) and torch.equal(rec["image"], real.decode(rec["latent"]))
    assert rec["image"].shape == image.shape


def test_edit_image_cli_proxnpi(tmp_path):
    from PIL import Image
    src = tmp_path / "in.png"
    Image.fromarray((np.random.default_rng(0).random((96, 96, 3)) * 255).astype(np.uint8)).save(src)
    out = tmp_path / "out.png"
    r = subprocess.run([sys.executable, str(ROOT / "eta-inversion_amd" / "edit_image.py"), "--input", str(src), "--source_prompt", SRC,
                        "--target_prompt", TGT, "--output", str(out), "--inv_method", "proxnpi", "--edit_method", "simple", "--steps", "3",
                        "--prec", "fp16"], capture_output=True, text=True, timeout=900,
                       env={**__import__("os").environ, "PYTHONPATH": str(ROOT / "eta-inversion_amd")})
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Saved result to" in r.stdout and "Took" in r.stdout
    assert out.exists() and (tmp_path / "out_inv.png").exists()
    assert Image.open(out).size == (512, 512)
